"""IP-Adapter image prompts for the SD1.5 pipelines: the checkpoint parser and the loader mixin.

Only the base layout is taken (ip-adapter_sd15, ip-adapter_sd15_light): the linear ImageProjection with ``num_tokens`` image tokens and
one ``to_k_ip`` / ``to_v_ip`` pair per cross-attention block of the UNet.  A checkpoint comes nested, as the IP-Adapter ``.bin`` files
are (``{"image_proj": {...}, "ip_adapter": {...}}``), or flattened, as their ``.safetensors`` conversions are
(``image_proj.proj.weight``, ``ip_adapter.1.to_k_ip.weight``, ...).  ``ip_adapter.{id}`` carries ``id = 2 j + 1`` for the UNet's
cross-attention blocks j in diffusers' attention-processor order: the blocks of the input side, then those of the output side, then the
middle block (id 31 for SD1.5).  Neither diffusers, the IP-Adapter package nor a published checkpoint was at hand when this was written:
that order and byte parity with diffusers are unpinned.

Everything else is refused with a NotImplementedError that names the offending key: Resampler projections ("plus"), the full-face MLP
projection, FaceID (LoRA keys), SDXL widths, several adapters at once, several images per adapter."""
import contextlib
import re
from typing import Dict, List, Mapping, Tuple

import numpy as np

from . import weights as W
from .weights import ModelConfig

_IP_KEY = re.compile(r"^ip_adapter\.(\d+)\.(to_k_ip|to_v_ip)\.weight$")
_PROJ_KEYS = ("image_proj.proj.weight", "image_proj.proj.bias", "image_proj.norm.weight", "image_proj.norm.bias")


def block_widths(cfg: ModelConfig) -> List[int]:
    """Channels C_j of the UNet's cross-attention blocks j in processor order: input blocks, output blocks, middle block."""
    enc = [b["cout"] for b in W.encoder_layout(cfg) if b["attn"]]
    dec = [b["cout"] for b in W.decoder_layout(cfg) if b["attn"]]
    return enc + dec + [cfg.model_channels * cfg.channel_mult[-1]]


def block_prefixes(cfg: ModelConfig, prefix: str = W.UNET_PREFIX) -> List[str]:
    """The state-dict prefix of the SpatialTransformer of block j, same order."""
    enc = [f"{prefix}input_blocks.{i}.1." for i, b in enumerate(W.encoder_layout(cfg)) if b["attn"]]
    dec = [f"{prefix}output_blocks.{i}.1." for i, b in enumerate(W.decoder_layout(cfg)) if b["attn"]]
    return enc + dec + [f"{prefix}middle_block.1."]


def param_shapes(cfg: ModelConfig, num_tokens: int, embed_dim: int) -> Dict[str, Tuple[int, ...]]:
    """Every tensor of the adapter under its flattened checkpoint name (what Engine.configure_ip_adapter registers)."""
    D = cfg.context_dim
    out = {"image_proj.proj.weight": (num_tokens * D, embed_dim), "image_proj.proj.bias": (num_tokens * D,),
           "image_proj.norm.weight": (D,), "image_proj.norm.bias": (D,)}
    for j, c in enumerate(block_widths(cfg)):
        out[f"ip_adapter.{2 * j + 1}.to_k_ip.weight"] = (c, D)
        out[f"ip_adapter.{2 * j + 1}.to_v_ip.weight"] = (c, D)
    return out


def _read(src) -> Dict[str, np.ndarray]:
    """path or mapping -> flat {name: float32 array}; .safetensors through lora.py's reader, anything else through torch.load"""
    from . import lora as L
    if isinstance(src, (list, tuple)):
        if len(src) != 1:
            raise NotImplementedError(f"{len(src)} IP-Adapters given: one adapter at a time (entry 1 is the first one too many)")
        src = src[0]
    if not isinstance(src, Mapping):
        if str(src).endswith(".safetensors"):
            return L._load(src)
        import torch
        src = torch.load(str(src), map_location="cpu", weights_only=True)
    flat = {}
    for k, v in src.items():
        if isinstance(v, Mapping):      # the nested layout: one level of "image_proj" / "ip_adapter"
            for k2, v2 in v.items():
                flat[f"{k}.{k2}"] = v2
        else:
            flat[str(k)] = v
    return L._load(flat)


def _refuse(key: str, what: str):
    raise NotImplementedError(f"IP-Adapter checkpoint key '{key}': {what} is not supported (only the base ip-adapter_sd15 layout: linear "
                              "image_proj.proj + image_proj.norm, ip_adapter.{id}.to_k_ip / to_v_ip)")


def parse_ip_adapter(src, cfg: ModelConfig = W.SD15) -> Tuple[int, int, Dict[str, np.ndarray]]:
    """(num_tokens, embed_dim, {flattened name: float32 array}) of a base-layout IP-Adapter for `cfg`, or NotImplementedError naming the
    key that shows another layout."""
    sd = _read(src)
    D = cfg.context_dim
    widths = block_widths(cfg)
    for k in sorted(sd):
        if k in _PROJ_KEYS:
            continue
        m = _IP_KEY.match(k)
        if m:
            i = int(m.group(1))
            if i % 2 == 0 or i // 2 >= len(widths):
                _refuse(k, f"an adapter id outside 1, 3, .. {2 * len(widths) - 1} (another UNet: SDXL has 70 attention blocks)")
            shp = tuple(sd[k].shape)
            if shp != (widths[i // 2], D):
                _refuse(k, f"shape {shp} where this UNet's block {i // 2} takes {(widths[i // 2], D)} (SDXL or another width)")
            continue
        if "lora" in k:
            _refuse(k, "FaceID (LoRA weights inside the adapter)")
        if k.startswith("image_proj.latents") or k.startswith("image_proj.layers") or k.startswith("image_proj.proj_in") \
                or k.startswith("image_proj.proj_out") or k.startswith("image_proj.norm_out") or "perceiver" in k:
            _refuse(k, 'the Resampler projection ("plus" adapters)')
        if re.match(r"^image_proj\.proj\.\d+\.", k) or k.startswith("image_proj.ff"):
            _refuse(k, "the MLP projection (full-face / FaceID adapters)")
        _refuse(k, "this tensor")
    want = [k for k in _PROJ_KEYS if k not in sd]
    want += [k for j in range(len(widths)) for k in (f"ip_adapter.{2 * j + 1}.to_k_ip.weight", f"ip_adapter.{2 * j + 1}.to_v_ip.weight") if k not in sd]
    if want:
        raise NotImplementedError(f"IP-Adapter checkpoint lacks '{want[0]}' ({len(want)} tensors of the base layout missing)")
    pw = sd["image_proj.proj.weight"]
    if pw.ndim != 2 or pw.shape[0] % D or pw.shape[0] // D < 1:
        _refuse("image_proj.proj.weight", f"shape {tuple(pw.shape)} (rows must be num_tokens x context_dim {D}: an SDXL adapter projects to 2048)")
    T, Edim = pw.shape[0] // D, int(pw.shape[1])
    for k, shp in param_shapes(cfg, T, Edim).items():
        if tuple(sd[k].shape) != shp:
            _refuse(k, f"shape {tuple(sd[k].shape)} where {shp} is expected")
    if T > 64:
        _refuse("image_proj.proj.weight", f"{T} image tokens (at most 64)")
    return T, Edim, sd


def synth_ip_adapter(cfg: ModelConfig, num_tokens: int = 4, embed_dim: int = 1024, seed: int = 4321, kv_gain: float = 1.0) -> Dict[str, np.ndarray]:
    """Seeded adapter weights in the flattened layout (tests, benchmarks): weights.synth_tensor's recipe per tensor, to_k_ip / to_v_ip
    multiplied by kv_gain."""
    out = {}
    for k, shp in param_shapes(cfg, num_tokens, embed_dim).items():
        kind = "w" if k.endswith("proj.weight") or "_ip." in k else "b" if k.endswith("proj.bias") else "gamma" if k.endswith("norm.weight") else "beta"
        t = W.synth_tensor(k, shp, kind, seed)
        out[k] = (t * np.float32(kv_gain)).astype(np.float32) if "_ip." in k else t
    return out


def nested(sd: Mapping) -> Dict[str, Dict[str, np.ndarray]]:
    """The flattened layout as the nested one of the .bin files."""
    out = {"image_proj": {}, "ip_adapter": {}}
    for k, v in sd.items():
        top, rest = k.split(".", 1)
        out[top][rest] = v
    return out


class IPAdapterMixin:
    """load_ip_adapter / set_ip_adapter_scale / unload_ip_adapter and the per-call image state of the SD1.5 pipelines.  The adapter
    lives in the engine (Engine.configure_ip_adapter): K / V of the image tokens are computed once per call, every UNet evaluation of
    the call adds the image term, and the state is dropped when the call ends, however it ends."""
    _ip_loaded = False

    def load_ip_adapter(self, path_or_dict, **kwargs):
        """A base-layout IP-Adapter (path to .safetensors / .bin, or a state dict, nested or flattened).  One adapter at a time."""
        if self._ip_loaded:
            raise NotImplementedError("an IP-Adapter is already loaded: more than one adapter is not supported (unload_ip_adapter first)")
        T, Edim, sd = parse_ip_adapter(path_or_dict, self.engine.cfg)
        self.engine.configure_ip_adapter(T, Edim)
        self.engine.load_state_dict(sd, strict=False)
        if self.engine.ip_adapter_weights_missing():
            raise ValueError(f"{self.engine.ip_adapter_weights_missing()} IP-Adapter tensors missing after load_ip_adapter")
        self.engine.ip_adapter_set_scale(1.0)
        self._ip_loaded = True

    def set_ip_adapter_scale(self, scale):
        """One float, or one per cross-attention block of the UNet (16, attention-processor order)."""
        if not self._ip_loaded:
            raise ValueError("set_ip_adapter_scale needs an adapter (load_ip_adapter)")
        if isinstance(scale, (list, tuple)) and len(scale) == 1 and isinstance(scale[0], (list, tuple)):
            scale = scale[0]                     # diffusers' one-list-per-adapter form
        self.engine.ip_adapter_set_scale(scale)

    def unload_ip_adapter(self):
        """The pipeline forgets the adapter: ip_adapter_image raises again and no image is ever set, so the engine runs as without one.
        The engine's registry keeps the tensors: loading an adapter of the same (num_tokens, embed_dim) again overwrites them, one of
        another shape needs a new engine (Engine.configure_ip_adapter says so)."""
        if self._ip_loaded:
            self.engine.ip_adapter_clear_image()
        self._ip_loaded = False

    # ------------------------------------------------------------------ per call
    @contextlib.contextmanager
    def _ip_image_of_call(self, ip_adapter_image, ip_adapter_image_embeds, prompt, prompt_embeds, num_images_per_prompt, guidance_scale):
        """Around the body of a pipeline call: nothing without the two arguments; NotImplementedError for them without a loaded adapter;
        else the image set in the engine for the body and cleared after it, however it ends."""
        if ip_adapter_image is None and ip_adapter_image_embeds is None:
            yield
            return
        if not self._ip_loaded:
            what = "ip_adapter_image" if ip_adapter_image is not None else "ip_adapter_image_embeds"
            raise NotImplementedError(f"{what} needs an IP-Adapter (load_ip_adapter); none is loaded")
        if prompt is not None:
            batch_size = 1 if isinstance(prompt, str) else len(prompt)
        else:
            batch_size = prompt_embeds.shape[0]
        emb, neg = self._ip_embeds_of_call(ip_adapter_image, ip_adapter_image_embeds, batch_size, num_images_per_prompt, guidance_scale > 1)
        self.engine.ip_adapter_set_image(emb, neg)
        try:
            yield
        finally:
            self.engine.ip_adapter_clear_image()

    def _ip_embeds_of_call(self, ip_adapter_image, ip_adapter_image_embeds, batch_size, num_images_per_prompt, do_cfg):
        """(cond [Bi, E], negative [Bi, E] or None) with Bi = 1 or the sampling batch."""
        B = batch_size * num_images_per_prompt
        if ip_adapter_image_embeds is not None:
            emb = ip_adapter_image_embeds
            if isinstance(emb, (list, tuple)):
                if len(emb) != 1:
                    raise NotImplementedError(f"ip_adapter_image_embeds: {len(emb)} entries, one per adapter and only one adapter is supported")
                emb = emb[0]
            emb = np.asarray(emb.detach().float().cpu().numpy() if type(emb).__module__.startswith("torch") else emb, np.float32)
            if emb.ndim == 3:
                if emb.shape[1] != 1:
                    raise NotImplementedError(f"ip_adapter_image_embeds of shape {emb.shape}: more than one image per adapter is not supported")
                emb = emb[:, 0]
            if emb.ndim != 2:
                raise ValueError(f"ip_adapter_image_embeds must be [B, E] or [B, 1, E], got {emb.shape}")
            R, neg = emb.shape[0], None
            # under guidance 2 B (or 2 x prompts, or 2 x 1) rows are diffusers' [negative ; positive], split by chunk(2); B (or prompts, or 1)
            # rows are the positive half alone and the negative half is the zero embedding
            if do_cfg and (R in (2 * B, 2 * batch_size) or (R == 2 and R not in (B, batch_size))):
                neg, emb = emb[:R // 2], emb[R // 2:]
        else:
            img = ip_adapter_image
            if isinstance(img, (list, tuple)):
                if len(img) != 1:
                    raise NotImplementedError(f"ip_adapter_image: {len(img)} entries, one per adapter and only one adapter is supported")
                img = img[0]
                if isinstance(img, (list, tuple)):
                    if len(img) != 1:
                        raise NotImplementedError(f"ip_adapter_image: {len(img)} images for one adapter; one image per adapter is supported")
                    img = img[0]
            emb, neg = self.encode_image(img, None, 1, None)
            emb, neg = np.asarray(emb, np.float32), np.asarray(neg, np.float32)
            if emb.shape[0] != 1:
                raise NotImplementedError(f"ip_adapter_image: {emb.shape[0]} images for one adapter; one image per adapter is supported")
        r = emb.shape[0]
        if r == batch_size and r != B:
            emb = np.repeat(emb, num_images_per_prompt, axis=0)
            neg = None if neg is None else np.repeat(neg, num_images_per_prompt, axis=0)
        elif r not in (1, B):
            raise ValueError(f"IP-Adapter: {r} image embeddings for a sampling batch of {B} (give 1, for every sample, or one per sample)")
        return np.ascontiguousarray(emb), None if neg is None else np.ascontiguousarray(neg)
