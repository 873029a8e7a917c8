"""Model configuration, parameter inventory and the synthetic-weight recipe.

The engine consumes weights under the reference's checkpoint names
(``model.diffusion_model.*`` for the SD1.5 UNet, ``control_model.*`` for the
Prompt-Diffusion ControlNet; reference ``tool_add_control.py:36-45``,
``cldm/model.py:12-21``).  ``param_spec`` enumerates every tensor the two
networks own, in the order the reference constructors create them
(``cldm/cldm.py:48-297`` and ``ldm/modules/diffusionmodules/openaimodel.py:442-736``),
so a checkpoint state-dict walk, the synthetic recipe and the engine's own
registry (``pd_param_name``) can be cross-checked by name and shape.

No trained checkpoint exists offline; ``synth_state_dict`` generates seeded
values, one independent Philox stream per tensor keyed by crc32(name), so any
subset can be regenerated on any host (the GPU box included) without torch.
"""
from __future__ import annotations

import dataclasses
import zlib
from typing import Dict, Iterator, List, Sequence, Tuple

import numpy as np

UNET_PREFIX = "model.diffusion_model."
CNET_PREFIX = "control_model."


@dataclasses.dataclass(frozen=True)
class ModelConfig:
    """Hyper-parameters of ``models/cldm_v15.yaml:30-62`` (defaults = SD1.5)."""

    in_channels: int = 4
    out_channels: int = 4
    hint_channels: int = 6      # example pair (two RGB images), cldm_v15.yaml:34
    query_channels: int = 3     # cldm/cldm.py:166
    model_channels: int = 320
    channel_mult: Tuple[int, ...] = (1, 2, 4, 4)
    num_res_blocks: int = 2
    attention_resolutions: Tuple[int, ...] = (4, 2, 1)
    num_heads: int = 8
    context_dim: int = 768
    context_len: int = 77
    hint_widths: Tuple[int, ...] = (16, 16, 32, 32, 96, 96, 256)  # cldm/cldm.py:147-163
    # schedule, cldm_v15.yaml:4-8
    timesteps: int = 1000
    linear_start: float = 0.00085
    linear_end: float = 0.0120

    # first-stage KL-VAE decoder, models/cldm_v15.yaml:64-85 (vae_ch = 0: not built)
    vae_ch: int = 128
    vae_ch_mult: Tuple[int, ...] = (1, 2, 4, 4)
    vae_num_res_blocks: int = 2
    vae_out_ch: int = 3
    scale_factor: float = 0.18215       # cldm_v15.yaml:17
    # first-stage KL-VAE encoder (Encoder + quant_conv, ldm/models/autoencoder.py:31-33): opt-in, same vae_* hyper-parameters
    vae_encoder: bool = False

    # cond-stage CLIP text transformer (FrozenCLIPEmbedder -> CLIPTextModel "openai/clip-vit-large-patch14",
    # ldm/modules/encoders/modules.py:88-131): width = context_dim, length = context_len (text_layers = 0: not built)
    text_vocab: int = 49408
    text_layers: int = 12
    text_heads: int = 12
    text_ff: int = 3072

    # HED edge detector (annotator/hed/__init__.py): opt-in, fixed architecture, registered through pd_hed_configure
    hed: bool = False
    # M-LSD line detector (annotator/mlsd): opt-in, fixed architecture, registered through pd_mlsd_configure
    mlsd: bool = False
    # CLIP image towers (ClipVisionConfig, at most two: image_encoder / the safety checker's): opt-in, registered through
    # pd_clip_vision_configure; safety_checker = True also registers StableDiffusionSafetyChecker's buffers (pd_safety_configure)
    clip_vision: Tuple = ()
    safety_checker: bool = False
    # (num_tokens, embed_dim) of an IP-Adapter (pd_ip_adapter_configure), or () for none
    ip_adapter: Tuple = ()

    @property
    def time_embed_dim(self) -> int:
        return 4 * self.model_channels


SD15 = ModelConfig()

OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
SAFETY_PREFIX = "safety_checker.vision_model."
IMAGE_ENCODER_PREFIX = "image_encoder."


@dataclasses.dataclass(frozen=True)
class ClipVisionConfig:
    """transformers' CLIPVisionConfig + projection_dim, and where the tower sits in a diffusers checkpoint (`prefix`).  stream_f32:
    the residual stream stays in float32 in every precision mode (image_encoder); False keeps the engine's stream type (safety tower)."""

    hidden: int = 1024
    layers: int = 24
    heads: int = 16
    ff: int = 4096
    patch: int = 14
    image_size: int = 224
    proj_dim: int = 768
    act: str = "quick_gelu"             # or "gelu" (erf)
    eps: float = 1e-5
    prefix: str = IMAGE_ENCODER_PREFIX
    stream_f32: bool = True
    mean: Tuple[float, float, float] = OPENAI_CLIP_MEAN
    std: Tuple[float, float, float] = OPENAI_CLIP_STD

    @property
    def patches(self) -> int:
        return (self.image_size // self.patch) ** 2

    @property
    def outer_prefix(self) -> str:
        """Where visual_projection lives: the prefix without a trailing 'vision_model.'"""
        return self.prefix[:-len("vision_model.")] if self.prefix.endswith("vision_model.") else self.prefix


# openai/clip-vit-large-patch14 inside StableDiffusionSafetyChecker; laion/CLIP-ViT-H-14 (the IP-Adapter image_encoder)
CLIP_VIT_L14_SAFETY = ClipVisionConfig(prefix=SAFETY_PREFIX, stream_f32=False)
CLIP_VIT_H14 = ClipVisionConfig(hidden=1280, layers=32, heads=16, ff=5120, proj_dim=1024, act="gelu", prefix=IMAGE_ENCODER_PREFIX)


def clip_vision_param_shapes(cfg: ClipVisionConfig) -> Dict[str, Tuple[int, ...]]:
    """Name -> shape of one tower, in registry order: transformers' CLIPVisionModelWithProjection.state_dict() under cfg.prefix."""
    C, F, p = cfg.hidden, cfg.ff, cfg.patch
    V = cfg.prefix + "vision_model."
    out = {V + "embeddings.class_embedding": (C,), V + "embeddings.patch_embedding.weight": (C, 3, p, p),
           V + "embeddings.position_embedding.weight": (cfg.patches + 1, C), V + "pre_layrnorm.weight": (C,), V + "pre_layrnorm.bias": (C,)}
    for i in range(cfg.layers):
        L = f"{V}encoder.layers.{i}."
        for nm in ("k_proj", "v_proj", "q_proj", "out_proj"):
            out[L + f"self_attn.{nm}.weight"] = (C, C)
            out[L + f"self_attn.{nm}.bias"] = (C,)
        out[L + "layer_norm1.weight"] = (C,)
        out[L + "layer_norm1.bias"] = (C,)
        out[L + "mlp.fc1.weight"] = (F, C)
        out[L + "mlp.fc1.bias"] = (F,)
        out[L + "mlp.fc2.weight"] = (C, F)
        out[L + "mlp.fc2.bias"] = (C,)
        out[L + "layer_norm2.weight"] = (C,)
        out[L + "layer_norm2.bias"] = (C,)
    out[V + "post_layernorm.weight"] = (C,)
    out[V + "post_layernorm.bias"] = (C,)
    out[cfg.outer_prefix + "visual_projection.weight"] = (cfg.proj_dim, C)
    return out


def safety_param_shapes(proj_dim: int) -> Dict[str, Tuple[int, ...]]:
    """StableDiffusionSafetyChecker's four buffers."""
    return {"safety_checker.concept_embeds": (17, proj_dim), "safety_checker.special_care_embeds": (3, proj_dim),
            "safety_checker.concept_embeds_weights": (17,), "safety_checker.special_care_embeds_weights": (3,)}
# A reduced network with the same topology (4 levels, attention at ds 1/2/4,
# 8 heads) used by fast parity tests: channels 64/128/256/256, dh 8/16/32.
TINY = ModelConfig(model_channels=64, context_dim=96, context_len=77,
                   hint_widths=(8, 8, 16, 16, 24, 24, 32), vae_ch=32,
                   text_vocab=1000, text_layers=2, text_heads=3, text_ff=192)

Spec = Tuple[str, Tuple[int, ...], str]  # (name, shape, kind)


def _res(prefix: str, cin: int, cout: int, temb: int) -> Iterator[Spec]:
    # ResBlock, openaimodel.py:200-240
    yield prefix + "in_layers.0.weight", (cin,), "gamma"
    yield prefix + "in_layers.0.bias", (cin,), "beta"
    yield prefix + "in_layers.2.weight", (cout, cin, 3, 3), "w"
    yield prefix + "in_layers.2.bias", (cout,), "b"
    yield prefix + "emb_layers.1.weight", (cout, temb), "w"
    yield prefix + "emb_layers.1.bias", (cout,), "b"
    yield prefix + "out_layers.0.weight", (cout,), "gamma"
    yield prefix + "out_layers.0.bias", (cout,), "beta"
    yield prefix + "out_layers.3.weight", (cout, cout, 3, 3), "w"
    yield prefix + "out_layers.3.bias", (cout,), "b"
    if cin != cout:
        yield prefix + "skip_connection.weight", (cout, cin, 1, 1), "w"
        yield prefix + "skip_connection.bias", (cout,), "b"


def _st(prefix: str, ch: int, ctx: int) -> Iterator[Spec]:
    # SpatialTransformer (depth 1, use_linear False), attention.py:287-319
    yield prefix + "norm.weight", (ch,), "gamma"
    yield prefix + "norm.bias", (ch,), "beta"
    yield prefix + "proj_in.weight", (ch, ch, 1, 1), "w"
    yield prefix + "proj_in.bias", (ch,), "b"
    t = prefix + "transformer_blocks.0."
    yield t + "attn1.to_q.weight", (ch, ch), "w"
    yield t + "attn1.to_k.weight", (ch, ch), "w"
    yield t + "attn1.to_v.weight", (ch, ch), "w"
    yield t + "attn1.to_out.0.weight", (ch, ch), "w"
    yield t + "attn1.to_out.0.bias", (ch,), "b"
    yield t + "ff.net.0.proj.weight", (8 * ch, ch), "w"
    yield t + "ff.net.0.proj.bias", (8 * ch,), "b"
    yield t + "ff.net.2.weight", (ch, 4 * ch), "w"
    yield t + "ff.net.2.bias", (ch,), "b"
    yield t + "attn2.to_q.weight", (ch, ch), "w"
    yield t + "attn2.to_k.weight", (ch, ctx), "w"
    yield t + "attn2.to_v.weight", (ch, ctx), "w"
    yield t + "attn2.to_out.0.weight", (ch, ch), "w"
    yield t + "attn2.to_out.0.bias", (ch,), "b"
    for n in ("norm1", "norm2", "norm3"):
        yield t + n + ".weight", (ch,), "gamma"
        yield t + n + ".bias", (ch,), "beta"
    yield prefix + "proj_out.weight", (ch, ch, 1, 1), "w"
    yield prefix + "proj_out.bias", (ch,), "b"


def _conv(prefix: str, cin: int, cout: int, k: int) -> Iterator[Spec]:
    yield prefix + "weight", (cout, cin, k, k), "w"
    yield prefix + "bias", (cout,), "b"


def encoder_layout(cfg: ModelConfig) -> List[dict]:
    """The 12 input blocks shared by UNet and ControlNet (openaimodel.py:542-621).

    Each entry: kind 'conv_in' | 'res' | 'down', cin, cout, attn(bool), ds.
    """
    mc = cfg.model_channels
    blocks = [dict(kind="conv_in", cin=cfg.in_channels, cout=mc, attn=False, ds=1)]
    ch, ds = mc, 1
    for level, mult in enumerate(cfg.channel_mult):
        for _ in range(cfg.num_res_blocks):
            blocks.append(dict(kind="res", cin=ch, cout=mult * mc,
                               attn=ds in cfg.attention_resolutions, ds=ds))
            ch = mult * mc
        if level != len(cfg.channel_mult) - 1:
            blocks.append(dict(kind="down", cin=ch, cout=ch, attn=False, ds=ds))
            ds *= 2
    return blocks


def decoder_layout(cfg: ModelConfig) -> List[dict]:
    """The 12 output blocks (openaimodel.py:662-724): res(ch+skip -> mult*mc), attn, up."""
    mc = cfg.model_channels
    enc = encoder_layout(cfg)
    chans = [b["cout"] for b in enc]
    ch = enc[-1]["cout"]
    ds = 2 ** (len(cfg.channel_mult) - 1)
    out = []
    for level, mult in list(enumerate(cfg.channel_mult))[::-1]:
        for i in range(cfg.num_res_blocks + 1):
            ich = chans.pop()
            blk = dict(cin=ch + ich, skip=ich, cout=mc * mult,
                       attn=ds in cfg.attention_resolutions, up=False, ds=ds)
            ch = mc * mult
            if level and i == cfg.num_res_blocks:
                blk["up"] = True
                ds //= 2
            out.append(blk)
    return out


def _encoder_spec(prefix: str, cfg: ModelConfig) -> Iterator[Spec]:
    temb = cfg.time_embed_dim
    yield prefix + "time_embed.0.weight", (temb, cfg.model_channels), "w"
    yield prefix + "time_embed.0.bias", (temb,), "b"
    yield prefix + "time_embed.2.weight", (temb, temb), "w"
    yield prefix + "time_embed.2.bias", (temb,), "b"
    for i, b in enumerate(encoder_layout(cfg)):
        p = f"{prefix}input_blocks.{i}."
        if b["kind"] == "conv_in":
            yield from _conv(p + "0.", b["cin"], b["cout"], 3)
        elif b["kind"] == "res":
            yield from _res(p + "0.", b["cin"], b["cout"], temb)
            if b["attn"]:
                yield from _st(p + "1.", b["cout"], cfg.context_dim)
        else:
            yield from _conv(p + "0.op.", b["cin"], b["cout"], 3)


def _middle_spec(prefix: str, cfg: ModelConfig) -> Iterator[Spec]:
    ch = cfg.model_channels * cfg.channel_mult[-1]
    temb = cfg.time_embed_dim
    yield from _res(prefix + "middle_block.0.", ch, ch, temb)
    yield from _st(prefix + "middle_block.1.", ch, cfg.context_dim)
    yield from _res(prefix + "middle_block.2.", ch, ch, temb)


def unet_spec(cfg: ModelConfig, prefix: str = UNET_PREFIX) -> List[Spec]:
    out = list(_encoder_spec(prefix, cfg)) + list(_middle_spec(prefix, cfg))
    temb = cfg.time_embed_dim
    for i, b in enumerate(decoder_layout(cfg)):
        p = f"{prefix}output_blocks.{i}."
        out += list(_res(p + "0.", b["cin"], b["cout"], temb))
        j = 1
        if b["attn"]:
            out += list(_st(p + "1.", b["cout"], cfg.context_dim))
            j = 2
        if b["up"]:
            out += list(_conv(p + f"{j}.conv.", b["cout"], b["cout"], 3))
    mc = cfg.model_channels
    out += [(prefix + "out.0.weight", (mc,), "gamma"), (prefix + "out.0.bias", (mc,), "beta")]
    out += list(_conv(prefix + "out.2.", mc, cfg.out_channels, 3))
    return out


def hint_layout(cfg: ModelConfig, cin: int) -> List[dict]:
    """input_hint_block / input_cond_block: 8 convs (cldm/cldm.py:147-181)."""
    w = cfg.hint_widths
    chain = [(cin, w[0], 1), (w[0], w[1], 1), (w[1], w[2], 2), (w[2], w[3], 1),
             (w[3], w[4], 2), (w[4], w[5], 1), (w[5], w[6], 2), (w[6], cfg.model_channels, 1)]
    return [dict(idx=2 * i, cin=a, cout=b, stride=s, silu=i < 7) for i, (a, b, s) in enumerate(chain)]


def controlnet_spec(cfg: ModelConfig, prefix: str = CNET_PREFIX) -> List[Spec]:
    out = list(_encoder_spec(prefix, cfg))
    enc = encoder_layout(cfg)
    for i, b in enumerate(enc):
        out += list(_conv(f"{prefix}zero_convs.{i}.0.", b["cout"], b["cout"], 1))
    for name, cin in (("input_hint_block", cfg.hint_channels), ("input_cond_block", cfg.query_channels)):
        for l in hint_layout(cfg, cin):
            out += list(_conv(f"{prefix}{name}.{l['idx']}.", l["cin"], l["cout"], 3))
    out += list(_middle_spec(prefix, cfg))
    ch = cfg.model_channels * cfg.channel_mult[-1]
    out += list(_conv(prefix + "middle_block_out.0.", ch, ch, 1))
    return out


def param_spec(cfg: ModelConfig) -> List[Spec]:
    return unet_spec(cfg) + controlnet_spec(cfg)


VAE_PREFIX = "first_stage_model."


def vae_layout(cfg: ModelConfig) -> List[dict]:
    """Decoder.up levels in EXECUTION order (highest i_level first), ldm/modules/diffusionmodules/model.py:588-606."""
    nres = len(cfg.vae_ch_mult)
    block_in = cfg.vae_ch * cfg.vae_ch_mult[-1]
    out = []
    for i_level in reversed(range(nres)):
        block_out = cfg.vae_ch * cfg.vae_ch_mult[i_level]
        blocks = []
        for _ in range(cfg.vae_num_res_blocks + 1):
            blocks.append((block_in, block_out))
            block_in = block_out
        out.append(dict(level=i_level, blocks=blocks, upsample=i_level != 0, ch=block_in))
    return out


def _vres(prefix: str, cin: int, cout: int) -> Iterator[Spec]:
    # ResnetBlock (temb_channels = 0), model.py:82-141
    yield prefix + "norm1.weight", (cin,), "gamma"
    yield prefix + "norm1.bias", (cin,), "beta"
    yield from _conv(prefix + "conv1.", cin, cout, 3)
    yield prefix + "norm2.weight", (cout,), "gamma"
    yield prefix + "norm2.bias", (cout,), "beta"
    yield from _conv(prefix + "conv2.", cout, cout, 3)
    if cin != cout:
        yield from _conv(prefix + "nin_shortcut.", cin, cout, 1)


def vae_spec(cfg: ModelConfig, prefix: str = VAE_PREFIX) -> List[Spec]:
    """post_quant_conv + Decoder parameters in the reference's registration order
    (ldm/models/autoencoder.py:34, model.py:546-653): decoder first (conv_in, mid, up.0..3, norm_out, conv_out),
    then post_quant_conv."""
    if cfg.vae_ch <= 0:
        return []
    d = prefix + "decoder."
    top = cfg.vae_ch * cfg.vae_ch_mult[-1]
    out: List[Spec] = list(_conv(d + "conv_in.", cfg.in_channels, top, 3))
    out += list(_vres(d + "mid.block_1.", top, top))
    out += [(d + "mid.attn_1.norm.weight", (top,), "gamma"), (d + "mid.attn_1.norm.bias", (top,), "beta")]
    for n in ("q", "k", "v", "proj_out"):
        out += list(_conv(d + f"mid.attn_1.{n}.", top, top, 1))
    out += list(_vres(d + "mid.block_2.", top, top))
    by_level = {l["level"]: l for l in vae_layout(cfg)}
    for lvl in range(len(cfg.vae_ch_mult)):          # module order: up.0 .. up.N-1
        l = by_level[lvl]
        for j, (ci, co) in enumerate(l["blocks"]):
            out += list(_vres(d + f"up.{lvl}.block.{j}.", ci, co))
        if l["upsample"]:
            out += list(_conv(d + f"up.{lvl}.upsample.conv.", l["ch"], l["ch"], 3))
    out += [(d + "norm_out.weight", (cfg.vae_ch,), "gamma"), (d + "norm_out.bias", (cfg.vae_ch,), "beta")]
    out += list(_conv(d + "conv_out.", cfg.vae_ch, cfg.vae_out_ch, 3))
    out += list(_conv(prefix + "post_quant_conv.", cfg.in_channels, cfg.in_channels, 1))
    return out


def synth_vae_state_dict(cfg: ModelConfig, seed: int = 1234) -> Dict[str, np.ndarray]:
    return {n: synth_tensor(n, s, k, seed) for n, s, k in vae_spec(cfg)}


def _vattn(prefix: str, ch: int) -> Iterator[Spec]:
    # AttnBlock, model.py:144-168
    yield prefix + "norm.weight", (ch,), "gamma"
    yield prefix + "norm.bias", (ch,), "beta"
    for n in ("q", "k", "v", "proj_out"):
        yield from _conv(prefix + f"{n}.", ch, ch, 1)


def vae_encoder_spec(cfg: ModelConfig, prefix: str = VAE_PREFIX) -> List[Spec]:
    """Encoder + quant_conv parameters in the reference's registration order (model.py:452-506 with double_z and
    attn_resolutions = [], autoencoder.py:33): encoder.conv_in, down.0..N-1 (blocks, downsample.conv on all but the last),
    mid, norm_out, conv_out, then quant_conv.  Independent of ``cfg.vae_encoder`` (which only decides whether an engine
    builds it)."""
    if cfg.vae_ch <= 0:
        return []
    e = prefix + "encoder."
    z2 = 2 * cfg.in_channels
    out: List[Spec] = list(_conv(e + "conv_in.", cfg.vae_out_ch, cfg.vae_ch, 3))
    block_in = cfg.vae_ch
    nl = len(cfg.vae_ch_mult)
    for lvl, mult in enumerate(cfg.vae_ch_mult):
        block_out = cfg.vae_ch * mult
        for j in range(cfg.vae_num_res_blocks):
            out += list(_vres(e + f"down.{lvl}.block.{j}.", block_in, block_out))
            block_in = block_out
        if lvl != nl - 1:
            out += list(_conv(e + f"down.{lvl}.downsample.conv.", block_in, block_in, 3))
    out += list(_vres(e + "mid.block_1.", block_in, block_in))
    out += list(_vattn(e + "mid.attn_1.", block_in))
    out += list(_vres(e + "mid.block_2.", block_in, block_in))
    out += [(e + "norm_out.weight", (block_in,), "gamma"), (e + "norm_out.bias", (block_in,), "beta")]
    out += list(_conv(e + "conv_out.", block_in, z2, 3))
    out += list(_conv(prefix + "quant_conv.", z2, z2, 1))
    return out


def synth_vae_encoder_state_dict(cfg: ModelConfig, seed: int = 1234) -> Dict[str, np.ndarray]:
    return {n: synth_tensor(n, s, k, seed) for n, s, k in vae_encoder_spec(cfg)}


HED_PREFIX = "hed."
_HED_STAGES = (("One", 64, 2), ("Two", 128, 2), ("Thr", 256, 3), ("Fou", 512, 3), ("Fiv", 512, 3))


def hed_spec(prefix: str = HED_PREFIX) -> List[Spec]:
    """The 38 tensors of the HED ``Network`` (annotator/hed/__init__.py:13-67) in its state-dict order, under ``hed.`` + the
    module's own names: the VGG-16 trunk (13 conv3x3; ``Sequential`` indices 0, 2 in stage one and 1, 3(, 5) behind the
    MaxPool2d of the later stages), five conv1x1 score heads, the 5 -> 1 combine."""
    out: List[Spec] = []
    cin = 3
    for s, (tag, width, n) in enumerate(_HED_STAGES):
        for j in range(n):
            out += list(_conv(f"{prefix}netVgg{tag}.{2 * j + (1 if s else 0)}.", cin, width, 3))
            cin = width
    for tag, width, _ in _HED_STAGES:
        out += list(_conv(f"{prefix}netScore{tag}.", width, 1, 1))
    out += list(_conv(prefix + "netCombine.0.", 5, 1, 1))
    return out


def synth_hed_state_dict(seed: int = 1234) -> Dict[str, np.ndarray]:
    """Seeded HED weights.  The plain recipe saturates the detector (13 ReLU layers without a normalisation halve the activation
    power each, the score heads then see std ~ 26 and the sigmoid sits at 0), so the trunk weights carry the He gain sqrt(2),
    which keeps the activations level, and the score heads are scaled by 0.02, which leaves the side maps at std ~ 1."""
    sd = {}
    for n, s, k in hed_spec():
        x = synth_tensor(n, s, k, seed)
        if k == "w" and ".netVgg" in n:
            x = x * np.float32(np.sqrt(2.0))
        elif k == "w" and ".netScore" in n:
            x = x * np.float32(0.02)
        sd[n] = x
    return sd


def hed_key(name: str) -> str:
    """A HED tensor's name in the engine's registry from the checkpoint's ``module...`` key (network-bsds500.pth), ``Network``'s
    own ``net...`` key, or the registry name itself; raises KeyError for anything else."""
    k = name
    if k.startswith(HED_PREFIX):
        k = k[len(HED_PREFIX):]
    if k.startswith("module"):
        k = "net" + k[len("module"):]       # Network.__init__: strKey.replace('module', 'net')
    k = HED_PREFIX + k
    if k not in _HED_NAMES:
        raise KeyError(f"not a HED tensor: '{name}'")
    return k


_HED_NAMES = frozenset(n for n, _, _ in hed_spec())


MLSD_PREFIX = "mlsd."
_MLSD_SETTING = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1))   # t, c, n, s (mbv2_mlsd_large.py:173-182)
_MLSD_SKIP = (64, 32, 24, 16)    # in_c1 of blocks 15, 17, 19, 21
MLSD_BN_EPS = 1e-5


def _bn(prefix: str, c: int) -> Iterator[Spec]:
    yield prefix + "weight", (c,), "bn_gamma"
    yield prefix + "bias", (c,), "bn_beta"
    yield prefix + "running_mean", (c,), "bn_mean"
    yield prefix + "running_var", (c,), "bn_var"
    yield prefix + "num_batches_tracked", (), "bn_count"


def mlsd_layers() -> List[dict]:
    """Every conv of ``MobileV2_MLSD_Large`` in ``state_dict()`` order: conv (key prefix), bn (key prefix of the BatchNorm behind it,
    or None), cin, cout, k, groups, bias (the conv has one of its own)."""
    out = []
    f = "backbone.features."
    add = lambda conv, bn, cin, cout, k, groups=1, bias=False: out.append(dict(conv=conv, bn=bn, cin=cin, cout=cout, k=k, groups=groups, bias=bias))
    add(f + "0.0.", f + "0.1.", 4, 32, 3)
    cin, idx = 32, 1
    for t, c, n, s in _MLSD_SETTING:
        for i in range(n):
            p, hidden, j = f"{f}{idx}.conv.", cin * t, 0
            if t != 1:
                add(p + "0.0.", p + "0.1.", cin, hidden, 1)
                j = 1
            add(f"{p}{j}.0.", f"{p}{j}.1.", hidden, hidden, 3, groups=hidden)
            add(f"{p}{j + 1}.", f"{p}{j + 2}.", hidden, c, 1)
            cin, idx = c, idx + 1
    for j in range(4):
        a, b = f"block{15 + 2 * j}.", f"block{16 + 2 * j}."
        add(a + "conv1.0.", a + "conv1.1.", 96 if j == 0 else 64, 64, 1, bias=True)
        add(a + "conv2.0.", a + "conv2.1.", _MLSD_SKIP[j], 64, 1, bias=True)
        add(b + "conv1.0.", b + "conv1.1.", 128, 128, 3, bias=True)
        add(b + "conv2.0.", b + "conv2.1.", 128, 64, 3, bias=True)
    add("block23.conv1.0.", "block23.conv1.1.", 64, 64, 3, bias=True)
    add("block23.conv2.0.", "block23.conv2.1.", 64, 64, 3, bias=True)
    add("block23.conv3.", None, 64, 16, 1, bias=True)
    return out


def mlsd_spec(prefix: str = MLSD_PREFIX) -> List[Spec]:
    """The checkpoint inventory of ``MobileV2_MLSD_Large`` (annotator/mlsd/models/mbv2_mlsd_large.py; mlsd_large_512_fp32.pth) in
    ``state_dict()`` order under ``mlsd.`` + its own keys: conv weights (and biases in the decoder blocks), and per BatchNorm
    weight / bias / running_mean / running_var / num_batches_tracked."""
    out: List[Spec] = []
    for L in mlsd_layers():
        out.append((prefix + L["conv"] + "weight", (L["cout"], L["cin"] // L["groups"], L["k"], L["k"]), "w"))
        if L["bias"]:
            out.append((prefix + L["conv"] + "bias", (L["cout"],), "b"))
        if L["bn"]:
            out += list(_bn(prefix + L["bn"], L["cout"]))
    return out


def mlsd_engine_spec(prefix: str = MLSD_PREFIX) -> List[Tuple[str, Tuple[int, ...]]]:
    """What the engine registers (pd_mlsd_configure): per conv its weight under the conv's key and one bias under the key of the
    BatchNorm's bias (block23.conv3: its own) -- the folded form ``fold_mlsd_state_dict`` produces."""
    out = []
    for L in mlsd_layers():
        out.append((prefix + L["conv"] + "weight", (L["cout"], L["cin"] // L["groups"], L["k"], L["k"])))
        out.append((prefix + (L["bn"] or L["conv"]) + "bias", (L["cout"],)))
    return out


# block23.conv3 of the seeded recipe: with the plain initialisation the reference's output is nearly flat (centre-logit std 0.017,
# displacements +-0.4), which no test could see an error in; tests/golden/make_golden_mlsd.py asserts what these reach
MLSD_HEAD_SCALE = {"center": 9.0, "center_shift": -1.9, "disp": 10.0, "other": 1.0}
MLSD_GAMMA = 0.8    # mean of the BatchNorm weights: with 1 / sqrt(running_var) ~ 1.3 the activations neither die nor grow through the 60 layers


def synth_mlsd_state_dict(seed: int = 1234) -> Dict[str, np.ndarray]:
    """Seeded M-LSD checkpoint.  The BatchNorm tensors are all away from their initial values: gamma = MLSD_GAMMA + 0.2 N, beta = 0.1 + 0.2 N, running_mean = 0.2 N, running_var = 0.5 + 0.09 N^2.
    block23.conv3's rows are scaled by MLSD_HEAD_SCALE (row 7: the centre logit, whose bias is also shifted; rows 8..11: the
    displacements)."""
    sd: Dict[str, np.ndarray] = {}
    for n, s, k in mlsd_spec():
        if k == "bn_count":
            sd[n] = np.zeros((), np.int64)
        elif k == "bn_gamma":
            sd[n] = np.float32(MLSD_GAMMA) + np.float32(2.0) * synth_tensor(n, s, "beta", seed)
        elif k == "bn_beta":
            sd[n] = np.float32(0.1) + np.float32(2.0) * synth_tensor(n, s, "beta", seed)
        elif k == "bn_mean":
            sd[n] = np.float32(2.0) * synth_tensor(n, s, "beta", seed)
        elif k == "bn_var":
            sd[n] = np.float32(0.5) + (np.float32(3.0) * synth_tensor(n, s, "beta", seed)) ** 2
        else:
            x = synth_tensor(n, s, k, seed)
            sd[n] = x
    w, b = sd[MLSD_PREFIX + "block23.conv3.weight"], sd[MLSD_PREFIX + "block23.conv3.bias"]
    scale = np.full(16, MLSD_HEAD_SCALE["other"], np.float32)
    scale[7] = MLSD_HEAD_SCALE["center"]
    scale[8:12] = MLSD_HEAD_SCALE["disp"]
    sd[MLSD_PREFIX + "block23.conv3.weight"] = w * scale[:, None, None, None]
    sd[MLSD_PREFIX + "block23.conv3.bias"] = b * scale
    sd[MLSD_PREFIX + "block23.conv3.bias"][7] += np.float32(MLSD_HEAD_SCALE["center_shift"])
    return sd


def fold_mlsd_state_dict(sd) -> Dict[str, np.ndarray]:
    """Checkpoint (keys with or without the ``mlsd.`` prefix; NumPy arrays or torch tensors) -> the engine's tensors
    (``mlsd_engine_spec``): every BatchNorm folded into the conv in front of it, in float64, rounded once to float32.
      s = gamma / sqrt(running_var + 1e-5);  weight' = weight * s[:, None, None, None];  bias' = (conv_bias - running_mean) * s + beta
    ``num_batches_tracked`` is ignored; a missing tensor raises KeyError, an unknown key ValueError."""
    src = {}
    for k, v in (sd.items() if hasattr(sd, "items") else sd):
        if hasattr(v, "detach"):
            v = v.detach().cpu().numpy()
        src[k if k.startswith(MLSD_PREFIX) else MLSD_PREFIX + k] = np.asarray(v)
    known = {n for n, _, _ in mlsd_spec()}
    extra = sorted(set(src) - known)
    if extra:
        raise ValueError(f"not an M-LSD tensor: '{extra[0]}'")
    get = lambda k: src[k].astype(np.float64)
    out: Dict[str, np.ndarray] = {}
    for L in mlsd_layers():
        conv = MLSD_PREFIX + L["conv"]
        w = get(conv + "weight")
        b = get(conv + "bias") if L["bias"] else np.zeros(L["cout"], np.float64)
        if L["bn"]:
            bn = MLSD_PREFIX + L["bn"]
            s = get(bn + "weight") / np.sqrt(get(bn + "running_var") + MLSD_BN_EPS)
            w = w * s[:, None, None, None]
            b = (b - get(bn + "running_mean")) * s + get(bn + "bias")
            out[conv + "weight"], out[bn + "bias"] = w.astype(np.float32), b.astype(np.float32)
        else:
            out[conv + "weight"], out[conv + "bias"] = w.astype(np.float32), b.astype(np.float32)
    return out


TEXT_PREFIX = "cond_stage_model.transformer.text_model."


def clip_text_spec(prefix: str, vocab: int, positions: int, hidden: int, ff: int, layers: int) -> List[Spec]:
    """Parameters of one transformers `CLIPTextModel` under `prefix` (its `text_model.`), in module order: embeddings,
    encoder.layers.i.{self_attn.{k,v,q,out}_proj, layer_norm1, mlp.fc1/fc2, layer_norm2}, final_layer_norm.  The SD1.5
    text transformer (text_spec) and the SD3 CLIP encoders (sd3.sd3_text_spec) are both this list."""
    C, F = hidden, ff
    out: List[Spec] = []
    out.append((prefix + "embeddings.token_embedding.weight", (vocab, C), "w"))
    out.append((prefix + "embeddings.position_embedding.weight", (positions, C), "w"))
    for i in range(layers):
        L = f"{prefix}encoder.layers.{i}."
        for nm in ("k_proj", "v_proj", "q_proj", "out_proj"):
            out.append((L + f"self_attn.{nm}.weight", (C, C), "w"))
            out.append((L + f"self_attn.{nm}.bias", (C,), "b"))
        out += [(L + "layer_norm1.weight", (C,), "gamma"), (L + "layer_norm1.bias", (C,), "beta")]
        out += [(L + "mlp.fc1.weight", (F, C), "w"), (L + "mlp.fc1.bias", (F,), "b")]
        out += [(L + "mlp.fc2.weight", (C, F), "w"), (L + "mlp.fc2.bias", (C,), "b")]
        out += [(L + "layer_norm2.weight", (C,), "gamma"), (L + "layer_norm2.bias", (C,), "beta")]
    out += [(prefix + "final_layer_norm.weight", (C,), "gamma"), (prefix + "final_layer_norm.bias", (C,), "beta")]
    return out


def text_spec(cfg: ModelConfig, prefix: str = TEXT_PREFIX) -> List[Spec]:
    """Parameters of the CLIP text transformer under the names the SD1.5 checkpoint stores them
    (`FrozenCLIPEmbedder.transformer` = transformers' `CLIPTextModel`, ldm/modules/encoders/modules.py:98)."""
    if cfg.text_layers <= 0:
        return []
    return clip_text_spec(prefix, cfg.text_vocab, cfg.context_len, cfg.context_dim, cfg.text_ff, cfg.text_layers)


def synth_text_state_dict(cfg: ModelConfig, seed: int = 1234) -> Dict[str, np.ndarray]:
    return {n: synth_tensor(n, s, k, seed) for n, s, k in text_spec(cfg)}


def synth_token_ids(cfg: ModelConfig, batch: int, seed: int = 7) -> np.ndarray:
    """Synthetic prompts: BOS, a run of random tokens, EOS padding to context_len (CLIPTokenizer pads with EOS for
    openai/clip-vit-large-patch14); int32 [batch, context_len]."""
    g = np.random.default_rng(seed)
    bos, eos = cfg.text_vocab - 2, cfg.text_vocab - 1
    ids = np.full((batch, cfg.context_len), eos, np.int32)
    ids[:, 0] = bos
    for b in range(batch):
        n = int(g.integers(3, cfg.context_len - 2))
        ids[b, 1:1 + n] = g.integers(0, cfg.text_vocab - 2, n)
    return ids


def num_params(cfg: ModelConfig) -> Tuple[int, int]:
    u = sum(int(np.prod(s)) for _, s, _ in unet_spec(cfg))
    c = sum(int(np.prod(s)) for _, s, _ in controlnet_spec(cfg))
    return u, c


def synth_tensor(name: str, shape: Sequence[int], kind: str, seed: int = 1234) -> np.ndarray:
    """Seeded value for one tensor (SURVEY.md §8d recipe).

    w: N(0, 1/fan_in); b: N(0, 0.02^2); gamma: 1 + N(0, 0.1^2); beta: N(0, 0.1^2).
    The reference's zero-initialised tensors (zero convs, ResBlock out conv,
    proj_out, hint-block last conv) get ordinary 'w'/'b' values,
    otherwise eps would be identically zero.
    """
    key = zlib.crc32(name.encode())
    rng = np.random.Generator(np.random.Philox(key=[seed, key]))
    x = rng.standard_normal(size=tuple(shape), dtype=np.float32)
    if kind == "w":
        fan_in = int(np.prod(shape[1:]))
        x *= np.float32(1.0 / np.sqrt(fan_in))
    elif kind == "b":
        x *= np.float32(0.02)
    elif kind == "gamma":
        x = np.float32(1.0) + np.float32(0.1) * x
    elif kind == "beta":
        x *= np.float32(0.1)
    else:
        raise ValueError(kind)
    return x


def synth_state_dict(cfg: ModelConfig, seed: int = 1234) -> Dict[str, np.ndarray]:
    return {n: synth_tensor(n, s, k, seed) for n, s, k in param_spec(cfg)}


def iter_synth(cfg: ModelConfig, seed: int = 1234):
    """Stream (name, array) pairs without holding the whole model in host memory."""
    for n, s, k in param_spec(cfg):
        yield n, synth_tensor(n, s, k, seed)


def synth_inputs(cfg: ModelConfig, batch: int, h: int, w: int, seed: int = 2023,
                 unit_range: bool = False) -> Dict[str, np.ndarray]:
    """Synthetic call inputs: x_T ~ N(0,1) seed 2023; ctx ~ N(0,1);
    pair/query ~ U(-1,1) ((L) convention) or U(0,1) ((D) convention)."""
    def g(tag):
        return np.random.Generator(np.random.Philox(key=[seed, zlib.crc32(tag.encode())]))
    lo = 0.0 if unit_range else -1.0
    return dict(
        x_T=g("x_T").standard_normal((batch, cfg.in_channels, h, w), dtype=np.float32),
        ctx_cond=g("ctx_cond").standard_normal((batch, cfg.context_len, cfg.context_dim), dtype=np.float32),
        ctx_uncond=g("ctx_uncond").standard_normal((batch, cfg.context_len, cfg.context_dim), dtype=np.float32),
        pair=g("pair").uniform(lo, 1.0, (batch, cfg.hint_channels, 8 * h, 8 * w)).astype(np.float32),
        query=g("query").uniform(lo, 1.0, (batch, cfg.query_channels, 8 * h, 8 * w)).astype(np.float32),
    )
