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
configurations map as well as SD1.5.  Formats this engine does not merge (LoHa, LoKr, DoRA, LoCon's Tucker middle factor,
SDXL's second text encoder, SD3 transformers) and targets it does not build raise ``NotImplementedError`` naming the first
such key; the ControlNet is not a LoRA target, as in diffusers.
"""
from __future__ import annotations

from typing import Dict, Mapping, Tuple, Union

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
