"""LoRA state dicts -> the engine's checkpoint tensor names.

``parse_lora`` reads a LoRA for SD1.5 (a dict of arrays, or a local ``.safetensors`` file) in any of the three common
layouts and returns ``{checkpoint_name: (up [N, r], down [r, K] or [r, cin, kh, kw], alpha)}`` under the names the engine
registers (``model.diffusion_model.*`` for the UNet, ``cond_stage_model.transformer.text_model.*`` for CLIP):

  * kohya: ``lora_unet_<module>`` / ``lora_te_<module>`` with ``.lora_up.weight``, ``.lora_down.weight`` and an optional
    ``.alpha`` (missing: alpha = rank); the module path has its dots replaced by underscores;
  * diffusers / PEFT: ``unet.<module>`` / ``text_encoder.<module>`` with ``.lora_A.weight`` (down) / ``.lora_B.weight`` (up);
  * legacy attention processors: ``<attention>.processor.to_{q,k,v,out}_lora.{down,up}.weight``.

The effective update of a tensor is ``scale * (alpha / r) * up @ down.reshape(r, -1)``, as in diffusers and kohya.  The
UNet's diffusers module names are mapped to the LDM names through the block layout of a ``ModelConfig``, so reduced
configurations map as well as SD1.5.  ``parse_lora`` is the strict plain-pair reader: LoHa, LoKr, DoRA, LoCon's Tucker middle
factor, SDXL's second text encoder, SD3 transformers and targets the engine does not build raise ``NotImplementedError`` naming
the first such key; the ControlNet is not a LoRA target, as in diffusers.

``parse_adapters`` (SD1.5) and ``parse_sd3_adapters`` (the SD3 transformer under diffusers' names, CLIP-L and CLIP-G) read the
same key layouts plus the LyCORIS suffixes (``lora_mid``, ``hada_*``, ``lokr_*``, ``dora_scale``) and PEFT's
``lora_magnitude_vector``, and return one ``Adapter`` record per tensor; ``lower`` turns a record into the operands of
``Engine.lora_add`` / ``Engine.lora_add_ex`` (DESIGN.md §7 "LoRA adapters" has the formulas).  Tucker cores and decomposed
Kronecker factors are folded here, in fp64, rounded once to fp32.  LyCORIS, PEFT and diffusers are not available to compare
against: that these formulas match those packages byte for byte is UNPINNED.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Callable, Dict, Mapping, Optional, Tuple, Union

import numpy as np

from . import weights as W
from .weights import ModelConfig

Triple = Tuple[np.ndarray, np.ndarray, float]

_RESNET = (("conv1", "in_layers.2"), ("conv2", "out_layers.3"), ("time_emb_proj", "emb_layers.1"),
           ("conv_shortcut", "skip_connection"))
_ATTN = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "ff.net.0.proj", "ff.net.2", "attn2.to_q", "attn2.to_k",
         "attn2.to_v", "attn2.to_out.0")
_TEXT = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "mlp.fc1", "mlp.fc2")

# key fragments of adapter types the merge does not express (checked first, in key order)
_REJECT = (("hada_", "LoHa"), ("lokr_", "LoKr"), ("lora_magnitude_vector", "DoRA"), ("dora_scale", "DoRA"),
           ("lora_mid", "LoCon with a Tucker middle factor"))
_REJECT_PREFIX = (("lora_te1_", "SDXL text encoders"), ("lora_te2_", "SDXL text encoders"), ("text_encoder_2.", "SDXL text encoders"),
                  ("transformer.", "SD3 transformer"), ("lora_transformer_", "SD3 transformer"), ("controlnet", "ControlNet"),
                  ("control_model", "ControlNet"))


def unet_module_map(cfg: ModelConfig) -> Dict[str, str]:
    """diffusers ``UNet2DConditionModel`` module name -> the engine's weight tensor name, for every matrix it builds."""
    P = W.UNET_PREFIX
    out: Dict[str, str] = {"conv_in": P + "input_blocks.0.0.weight", "conv_out": P + "out.2.weight",
                           "time_embedding.linear_1": P + "time_embed.0.weight", "time_embedding.linear_2": P + "time_embed.2.weight"}

    def res(d: str, l: str, skip: bool):
        for a, b in _RESNET:
            if a != "conv_shortcut" or skip:
                out[f"{d}.{a}"] = f"{l}.{b}.weight"

    def attn(d: str, l: str):
        out[f"{d}.proj_in"] = f"{l}.proj_in.weight"
        out[f"{d}.proj_out"] = f"{l}.proj_out.weight"
        for n in _ATTN:
            out[f"{d}.transformer_blocks.0.{n}"] = f"{l}.transformer_blocks.0.{n}.weight"

    nrb, levels = cfg.num_res_blocks, len(cfg.channel_mult)
    enc = W.encoder_layout(cfg)
    for i in range(levels):
        for j in range(nrb):
            k = (nrb + 1) * i + j + 1
            b = enc[k]
            res(f"down_blocks.{i}.resnets.{j}", f"{P}input_blocks.{k}.0", b["cin"] != b["cout"])
            if b["attn"]:
                attn(f"down_blocks.{i}.attentions.{j}", f"{P}input_blocks.{k}.1")
        if i != levels - 1:
            out[f"down_blocks.{i}.downsamplers.0.conv"] = f"{P}input_blocks.{(nrb + 1) * i + nrb + 1}.0.op.weight"
    res("mid_block.resnets.0", P + "middle_block.0", False)
    attn("mid_block.attentions.0", P + "middle_block.1")
    res("mid_block.resnets.1", P + "middle_block.2", False)
    dec = W.decoder_layout(cfg)
    for i in range(levels):
        for j in range(nrb + 1):
            k = (nrb + 1) * i + j
            b = dec[k]
            res(f"up_blocks.{i}.resnets.{j}", f"{P}output_blocks.{k}.0", b["cin"] != b["cout"])
            if b["attn"]:
                attn(f"up_blocks.{i}.attentions.{j}", f"{P}output_blocks.{k}.1")
            if b["up"]:
                out[f"up_blocks.{i}.upsamplers.0.conv"] = f"{P}output_blocks.{k}.{2 if b['attn'] else 1}.conv.weight"
    return out


def text_module_map(cfg: ModelConfig) -> Dict[str, str]:
    """transformers ``CLIPTextModel`` module name -> the engine's weight tensor name (attention and MLP matrices)."""
    out: Dict[str, str] = {}
    for i in range(cfg.text_layers):
        for n in _TEXT:
            out[f"text_model.encoder.layers.{i}.{n}"] = f"{W.TEXT_PREFIX}encoder.layers.{i}.{n}.weight"
    return out


def _load(src) -> Dict[str, np.ndarray]:
    if isinstance(src, Mapping):
        items = src.items()
    else:
        from safetensors.numpy import load_file
        items = load_file(str(src)).items()
    out = {}
    for k, v in items:
        if type(v).__module__.startswith("torch"):
            v = v.detach().float().cpu().numpy()
        out[str(k)] = np.asarray(v, dtype=np.float32)
    return out


def _split(key: str):
    """(family, module, role) of one key; role in up / down / alpha; None when the key is not a LoRA factor."""
    if key.startswith("lora_unet_") or key.startswith("lora_te_"):
        fam = "unet" if key.startswith("lora_unet_") else "te"
        mod, _, rest = key.partition(".")
        mod = mod[len("lora_unet_"):] if fam == "unet" else mod[len("lora_te_"):]
        role = {"lora_up.weight": "up", "lora_down.weight": "down", "alpha": "alpha"}.get(rest)
        return (fam + "_kohya", mod, role) if role else None
    fam = "unet"
    body = key
    if key.startswith("unet."):
        body = key[len("unet."):]
    elif key.startswith("text_encoder."):
        fam, body = "te", key[len("text_encoder."):]
    if ".processor." in body:   # legacy attention processors
        mod, _, rest = body.partition(".processor.")
        for proj, target in (("to_q", "to_q"), ("to_k", "to_k"), ("to_v", "to_v"), ("to_out", "to_out.0")):
            for sfx, role in (("_lora.down.weight", "down"), ("_lora.up.weight", "up")):
                if rest == proj + sfx:
                    return fam, f"{mod}.{target}", role
        return None
    for sfx, role in ((".lora_A.weight", "down"), (".lora_B.weight", "up"), (".lora.down.weight", "down"),
                      (".lora.up.weight", "up"), (".alpha", "alpha")):
        if body.endswith(sfx):
            return fam, body[:-len(sfx)], role
    return None


def parse_lora(src: Union[str, Mapping], cfg: ModelConfig = W.SD15) -> Dict[str, Triple]:
    """A LoRA state dict (or a local .safetensors path) -> {engine tensor name: (up [N, r], down, alpha)}."""
    sd = _load(src)
    for k in sd:
        for frag, what in _REJECT:
            if frag in k:
                raise NotImplementedError(f"LoRA key '{k}': {what} adapters are not supported (plain LoRA only)")
        for pre, what in _REJECT_PREFIX:
            if k.startswith(pre):
                raise NotImplementedError(f"LoRA key '{k}': {what} is not a LoRA target of this engine")
    unet, text = unet_module_map(cfg), text_module_map(cfg)
    kohya = {("unet", m.replace(".", "_")): n for m, n in unet.items()}
    kohya.update({("te", m.replace(".", "_")): n for m, n in text.items()})
    groups: Dict[str, Dict[str, np.ndarray]] = {}
    first_key: Dict[str, str] = {}
    for k, v in sd.items():
        s = _split(k)
        if s is None:
            raise NotImplementedError(f"LoRA key '{k}' is not a LoRA factor this engine can merge")
        fam, mod, role = s
        if fam.endswith("_kohya"):
            name = kohya.get((fam[:-len("_kohya")], mod))
        else:
            name = (unet if fam == "unet" else text).get(mod)
        if name is None:
            raise NotImplementedError(f"LoRA key '{k}': the engine builds no tensor for module '{mod}'")
        g = groups.setdefault(name, {})
        if role in g:
            raise ValueError(f"LoRA key '{k}': a second {role} factor for '{name}'")
        g[role] = v
        first_key.setdefault(name, k)
    out: Dict[str, Triple] = {}
    for name, g in groups.items():
        if "up" not in g or "down" not in g:
            raise ValueError(f"LoRA key '{first_key[name]}': '{name}' needs both an up and a down factor")
        up, down = g["up"], g["down"]
        if up.ndim == 4 and up.shape[2:] == (1, 1):
            up = up[:, :, 0, 0]
        if up.ndim != 2 or down.ndim not in (2, 4) or down.shape[0] != up.shape[1]:
            raise ValueError(f"LoRA key '{first_key[name]}': up {up.shape} / down {down.shape} are not a rank-r pair")
        alpha = float(g["alpha"].reshape(-1)[0]) if "alpha" in g else float(up.shape[1])
        out[name] = (np.ascontiguousarray(up), np.ascontiguousarray(down), alpha)
    return out


# ------------------------------------------------------------------------------------ every adapter form (parse_adapters)
_LYCO = ("hada_w1_a", "hada_w1_b", "hada_w2_a", "hada_w2_b", "hada_t1", "hada_t2", "lokr_w1", "lokr_w1_a", "lokr_w1_b", "lokr_w2",
         "lokr_w2_a", "lokr_w2_b", "lokr_t2")
_ROLES = {"lora_up.weight": "up", "lora_down.weight": "down", "lora_mid.weight": "mid", "alpha": "alpha", "dora_scale": "magnitude",
          "lora_magnitude_vector": "magnitude", "lora_magnitude_vector.weight": "magnitude", "lora_A.weight": "down",
          "lora_B.weight": "up", "lora.down.weight": "down", "lora.up.weight": "up", **{k: k[5:] for k in _LYCO}}
_LEGACY = {f"{p}_lora.{d}.weight": (t, d) for p, t in (("to_q", "to_q"), ("to_k", "to_k"), ("to_v", "to_v"), ("to_out", "to_out.0"))
           for d in ("down", "up")}


@dataclass
class Adapter:
    """What one adapter file holds for one tensor.  kind "lora": factors up, down (and mid: Tucker LoCon); "loha": w1_a, w1_b, w2_a,
    w2_b (and t1, t2); "lokr": w1 or w1_a + w1_b, and w2 or w2_a + w2_b (and t2).  alpha None: the file has none."""
    kind: str
    factors: Dict[str, np.ndarray] = field(default_factory=dict)
    alpha: Optional[float] = None
    magnitude: Optional[np.ndarray] = None
    key: str = ""      # the first key of the group, for messages


def _role_of(key: str):
    """(module path as written, role) of a dotted key, or None"""
    if ".processor." in key:
        mod, _, rest = key.partition(".processor.")
        if rest in _LEGACY:
            return f"{mod}.{_LEGACY[rest][0]}", _LEGACY[rest][1]
        return None
    best = None
    for sfx, role in _ROLES.items():
        if key.endswith("." + sfx) and (best is None or len(sfx) > len(best[0])):
            best = (sfx, role)
    return (key[:-len(best[0]) - 1], best[1]) if best else None


def effective_scale(a: Adapter) -> float:
    """alpha / r of the issue's rules: r is the rank of the factor that defines `dim`; a missing alpha, and a Kronecker adapter
    with no decomposed factor, give 1."""
    f = a.factors
    if a.kind == "lora":
        r = f["down"].shape[0]
    elif a.kind == "loha":
        r = f["w1_b"].shape[0]
    else:
        r = None
        if "w1_a" in f:
            r = f["w1_b"].shape[0]
        if "t2" in f:
            r = f["t2"].shape[0]
        elif "w2_a" in f:
            r = f["w2_b"].shape[0]
        if r is None:
            return 1.0
    return 1.0 if a.alpha is None else float(a.alpha) / float(r)


def tucker_fold(t: np.ndarray, wb: np.ndarray) -> np.ndarray:
    """sum_j t[i, j, y, x] wb[j, c] -> [r, cin, kh, kw]: the core folded into the input-side factor (fp64, rounded once)"""
    return np.einsum("ijyx,jc->icyx", t.astype(np.float64), wb.astype(np.float64)).astype(np.float32)


def _check_group(name: str, a: Adapter):
    """shape rules that need no knowledge of the target; the engine checks the rest against the tensor"""
    f, k = a.factors, a.key
    need = {"lora": [("up", "down")], "loha": [("w1_a", "w1_b", "w2_a", "w2_b")],
            "lokr": [("w1",), ("w1_a", "w1_b")]}[a.kind]
    if not any(all(r in f for r in alt) for alt in need):
        raise ValueError(f"LoRA key '{k}': '{name}' lacks a factor ({' / '.join('+'.join(alt) for alt in need)})")
    if a.kind == "loha" and ("t1" in f) != ("t2" in f):
        raise ValueError(f"LoRA key '{k}': '{name}' has one Tucker core of two")
    if a.kind == "lokr":
        if not ("w2" in f or ("w2_a" in f and "w2_b" in f)):
            raise ValueError(f"LoRA key '{k}': '{name}' lacks lokr_w2 (or lokr_w2_a + lokr_w2_b)")
        if "t2" in f and not ("w2_a" in f and "w2_b" in f):
            raise ValueError(f"LoRA key '{k}': '{name}' has lokr_t2 without lokr_w2_a + lokr_w2_b")
    if a.kind == "lora":
        up, down = f["up"], f["down"]
        if up.ndim == 4 and up.shape[2:] == (1, 1):
            up = up[:, :, 0, 0]
        if up.ndim != 2 or down.ndim not in (2, 4) or ("mid" not in f and down.shape[0] != up.shape[1]):
            raise ValueError(f"LoRA key '{k}': up {f['up'].shape} / down {down.shape} are not a rank-r pair")
        if "mid" in f:
            mid = f["mid"]
            if mid.ndim != 4 or down.ndim != 4 or down.shape[2:] != (1, 1) or mid.shape[0] != up.shape[1] or mid.shape[1] != down.shape[0]:
                raise ValueError(f"LoRA key '{k}': lora_mid {mid.shape} does not fit up {f['up'].shape} / down {down.shape}")


def _rows_of(a: Adapter) -> int:
    f = a.factors
    if a.kind == "lora":
        return f["up"].shape[0]
    if a.kind == "loha":
        return f["w1_a"].shape[1] if "t1" in f else f["w1_a"].shape[0]
    a_ = f["w1"].shape[0] if "w1" in f else f["w1_a"].shape[0]
    c_ = f["w2"].shape[0] if "w2" in f else (f["w2_a"].shape[1] if "t2" in f else f["w2_a"].shape[0])
    return a_ * c_


def _group(sd: Dict[str, np.ndarray], resolve: Callable[[str], Tuple[str, str]]) -> Dict[str, Adapter]:
    groups: Dict[str, Adapter] = {}
    mag_key: Dict[str, str] = {}
    for k, v in sd.items():
        name, role = resolve(k)
        kind = "loha" if "hada_" in k else "lokr" if "lokr_" in k else "lora" if role in ("up", "down", "mid") else None
        a = groups.setdefault(name, Adapter(kind="", key=k))
        if kind:
            if a.kind and a.kind != kind:
                raise ValueError(f"LoRA key '{k}': '{name}' mixes {a.kind} and {kind} factors")
            a.kind = kind
        if role == "alpha":
            a.alpha = float(v.reshape(-1)[0])
        elif role == "magnitude":
            if a.magnitude is not None:
                raise ValueError(f"LoRA key '{k}': a second magnitude for '{name}'")
            a.magnitude, mag_key[name] = v, k
        else:
            if role in a.factors:
                raise ValueError(f"LoRA key '{k}': a second {role} factor for '{name}'")
            a.factors[role] = v
    for name, a in groups.items():
        if not a.kind:
            raise ValueError(f"LoRA key '{a.key}': '{name}' has no factors")
        _check_group(name, a)
        if a.magnitude is not None:
            m, n = a.magnitude, _rows_of(a)
            if m.ndim >= 2 and m.shape[0] == 1 and m.size > 1:
                raise NotImplementedError(f"LoRA key '{mag_key[name]}': a magnitude {m.shape} on the input axis is not supported "
                                          "(output-axis DoRA only)")
            if m.size != n or m.shape[0] != n:
                raise ValueError(f"LoRA key '{mag_key[name]}': magnitude {m.shape} does not have the {n} output rows of '{name}'")
            a.magnitude = np.ascontiguousarray(m.reshape(-1))
    return groups


def _reject_prefixes(k: str, prefixes):
    for pre, what in prefixes:
        if k.startswith(pre):
            raise NotImplementedError(f"LoRA key '{k}': {what} is not a LoRA target of this engine")


def parse_adapters(src: Union[str, Mapping], cfg: ModelConfig = W.SD15) -> Dict[str, Adapter]:
    """An adapter state dict for SD1.5 (or a local .safetensors path) -> {engine tensor name: Adapter}: plain pairs, Tucker LoCon,
    LoHa, LoKr, each optionally under a DoRA magnitude.  Targets and refused prefixes are those of parse_lora."""
    sd = _load(src)
    unet, text = unet_module_map(cfg), text_module_map(cfg)
    kohya = {("unet", m.replace(".", "_")): n for m, n in unet.items()}
    kohya.update({("te", m.replace(".", "_")): n for m, n in text.items()})

    def resolve(k: str):
        _reject_prefixes(k, _REJECT_PREFIX)
        if k.startswith("lora_unet_") or k.startswith("lora_te_"):
            fam = "unet" if k.startswith("lora_unet_") else "te"
            mod, _, rest = k.partition(".")
            mod = mod[len("lora_unet_"):] if fam == "unet" else mod[len("lora_te_"):]
            if rest not in _ROLES:
                raise NotImplementedError(f"LoRA key '{k}' is not an adapter factor this engine can merge")
            name = kohya.get((fam, mod))
        else:
            s = _role_of(k)
            if s is None:
                raise NotImplementedError(f"LoRA key '{k}' is not an adapter factor this engine can merge")
            mod, rest = s[0], None
            fam = "unet"
            if mod.startswith("unet."):
                mod = mod[len("unet."):]
            elif mod.startswith("text_encoder."):
                fam, mod = "te", mod[len("text_encoder."):]
            name = (unet if fam == "unet" else text).get(mod)
        if name is None:
            raise NotImplementedError(f"LoRA key '{k}': the engine builds no tensor for module '{mod}'")
        return name, (_ROLES[rest] if rest is not None else s[1])

    return _group(sd, resolve)


_SD3_REJECT = (("lora_unet_", "kohya's SD3 layout (original MMDiT names, fused qkv)"), ("lora_transformer_", "kohya's SD3 layout"),
               ("lora_te", "kohya's SD3 text-encoder layout"), ("text_encoder_3.", "the T5 encoder"), ("controlnet", "ControlNet"),
               ("control_model", "ControlNet"))


def parse_sd3_adapters(src: Union[str, Mapping], cfg, text_cfg=None) -> Dict[str, Adapter]:
    """An adapter state dict for SD3 in diffusers / PEFT naming -> {engine tensor name: Adapter}.  ``transformer.<module>`` maps onto
    ``transformer.<module>.weight``, ``text_encoder.`` / ``text_encoder_2.`` onto CLIP-L / CLIP-G (``text_cfg``: the engine's
    SD3TextConfig, or None when it has no text encoders).  T5 and the ControlNet are not targets, as in SD3LoraLoaderMixin."""
    from . import sd3 as S
    sd = _load(src)
    shapes = {n: s for n, s in S.sd3_param_shapes(cfg).items() if n.startswith("transformer.")}
    if text_cfg is not None:
        shapes.update({n: s for n, s, _ in S.sd3_text_spec(text_cfg) if not n.startswith("text_encoder_3.")})
    targets = {n[:-len(".weight")]: n for n, s in shapes.items() if n.endswith(".weight") and len(s) >= 2}

    def resolve(k: str):
        _reject_prefixes(k, _SD3_REJECT)
        s = _role_of(k)
        if s is None:
            raise NotImplementedError(f"LoRA key '{k}' is not an adapter factor this engine can merge")
        name = targets.get(s[0])
        if name is None:
            raise NotImplementedError(f"LoRA key '{k}': the engine builds no tensor for module '{s[0]}'")
        return name, s[1]

    return _group(sd, resolve)


def lower(a: Adapter) -> Dict[str, Any]:
    """One record -> the operands of Engine.lora_add_ex: kind "pair" / "hada" / "kron", up, down, (up2, down2), scale, magnitude.
    Tucker cores and decomposed Kronecker factors are folded in fp64 and rounded once to fp32."""
    f = a.factors
    out: Dict[str, Any] = dict(scale=effective_scale(a), magnitude=a.magnitude)
    c = np.ascontiguousarray
    if a.kind == "lora":
        up, down = f["up"], f["down"]
        if up.ndim == 4:
            up = up[:, :, 0, 0]
        if "mid" in f:
            down = tucker_fold(f["mid"], down[:, :, 0, 0])
        out.update(kind="pair", up=c(up), down=c(down))
    elif a.kind == "loha":
        if "t1" in f:
            out.update(kind="hada", up=c(f["w1_a"].T), down=tucker_fold(f["t1"], f["w1_b"]), up2=c(f["w2_a"].T),
                       down2=tucker_fold(f["t2"], f["w2_b"]))
        else:
            out.update(kind="hada", up=c(f["w1_a"]), down=c(f["w1_b"]), up2=c(f["w2_a"]), down2=c(f["w2_b"]))
    else:
        f64 = lambda x: x.astype(np.float64)
        w1 = f["w1"] if "w1" in f else (f64(f["w1_a"]) @ f64(f["w1_b"])).astype(np.float32)
        if "w2" in f:
            w2 = f["w2"]
        elif "t2" in f:
            w2 = np.einsum("ijyx,ip,jq->pqyx", f64(f["t2"]), f64(f["w2_a"]), f64(f["w2_b"])).astype(np.float32)
        else:
            w2 = (f64(f["w2_a"]) @ f64(f["w2_b"])).astype(np.float32)     # [c, d * kh * kw]; the engine reads it as [c, d, kh, kw]
        out.update(kind="kron", up=c(w1), down=c(w2))
    return out


def add_to_engine(engine, adapter_id: int, name: str, a: Adapter) -> None:
    """Register one record: a plain pair goes through lora_add (with its alpha), everything else through lora_add_ex."""
    low = lower(a)
    if low["kind"] == "pair" and low["magnitude"] is None:
        alpha = a.alpha if a.alpha is not None else float(a.factors["down"].shape[0])
        engine.lora_add(adapter_id, name, low["up"], low["down"], alpha=alpha)
    else:
        engine.lora_add_ex(adapter_id, name, **low)
