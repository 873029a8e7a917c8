"""Host side of the SD3 / MMDiT variant of the path over the C ABI (pd_sd3_* in include/pdengine.h).

Mirrors, at the tensor level, what the reference's SD3 pipeline does per denoising step
(promptdiffusioncontrolnetpipeline_sd3.py:1192-1245): ControlNet (promptdiffusioncontrolnet_sd3.py:362-483), transformer
with ``block_controlnet_hidden_states``, classifier-free guidance, FlowMatchEuler step.  The boundary takes prompt embeddings and
condition LATENTS; SD3's VAE is opt-in on the same engine (``SD3Engine.configure_vae`` / ``vae_encode`` / ``vae_decode``: images in,
latents out and back).  The text encoders (CLIP-L, CLIP-G, T5; pipeline :238-545) are opt-in on the
same engine (``SD3Engine.configure_text`` / ``encode_prompt_ids``: token ids in, prompt embeddings out; tokenisation is the caller's).  PARITY UNPINNED (diffusers is absent offline): checked against oracle/sd3_oracle.py only."""
import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np

from . import engine as E
from . import weights as W


@dataclass(frozen=True)
class SD3Config:
    in_channels: int = 16
    out_channels: int = 16
    patch: int = 2
    heads: int = 24
    head_dim: int = 64
    layers: int = 24
    cn_layers: int = 6              # the reference class defaults to 18 (promptdiffusioncontrolnet_sd3.py:95); SD3 ControlNet
                                    # checkpoints ship 6 or 12 blocks
    joint_dim: int = 4096
    pooled_dim: int = 2048
    pos_embed_max_size: int = 192
    cn_pos_embed_max_size: int = 0  # 0: same as the transformer's
    force_zeros_for_pooled_projection: bool = True   # the reference class's default (promptdiffusioncontrolnet_sd3.py:108)
    # SD3.5-style blocks (promptdiffusioncontrolnet_sd3.py:104-105, :140-141): per-head RMSNorm of queries / keys, and a second,
    # image-only attention in the listed blocks (own lists for the transformer and the ControlNet)
    qk_norm: Optional[str] = None            # None or "rms_norm"
    dual_attention_layers: tuple = ()        # transformer blocks with attn2
    cn_dual_attention_layers: tuple = ()     # ControlNet blocks with attn2 (the reference class's dual_attention_layers)
    cn_single_blocks: bool = False           # the ControlNet built with joint_attention_dim=None: SD3SingleTransformerBlock, no
                                             # context stream / context_embedder (promptdiffusioncontrolnet_sd3.py:147-160)

    @property
    def hidden(self) -> int:
        return self.heads * self.head_dim


SD3_MEDIUM = SD3Config()
SD3_TINY = SD3Config(in_channels=4, out_channels=4, heads=2, head_dim=64, layers=3, cn_layers=2, joint_dim=96, pooled_dim=40,
                     pos_embed_max_size=12, cn_pos_embed_max_size=10)


class pd_sd3_config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("in_channels", "out_channels", "patch_size", "heads", "head_dim", "layers", "cn_layers",
                                         "joint_dim", "pooled_dim", "pos_embed_max_size", "cn_pos_embed_max_size",
                                         "cn_zero_pooled")] + \
               [("qk_norm", C.c_int32), ("dual_mask", C.c_uint32), ("cn_dual_mask", C.c_uint32), ("cn_single", C.c_int32)]


class pd_sd3_args(C.Structure):
    _fields_ = [("batch", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("context_len", C.c_int32), ("mem", C.c_int32),
                ("conditioning_scale", C.c_float),
                ("latents", C.c_void_p), ("timestep", C.c_void_p), ("context", C.c_void_p), ("pooled", C.c_void_p),
                ("cond", C.c_void_p), ("pair", C.c_void_p), ("cn_pooled", C.c_void_p), ("reserved", C.c_int64 * 3)]


class pd_sd3_loop_args(C.Structure):
    _fields_ = [("init_latents", C.c_void_p), ("mask", C.c_void_p), ("noise", C.c_void_p), ("flags", C.c_int32), ("reserved0", C.c_int32),
                ("reserved", C.c_int64 * 4)]


PD_INIT_PURE_NOISE, PD_XT_FROM_SEED = 1, 4      # pd_sd3_loop_args.flags (the SD1.5 loop's init_flags values)


def img2img_start(num_inference_steps: int, strength: float) -> int:
    """diffusers' SD3 img2img get_timesteps: the index t_start of the first kept step; the loop runs on sigmas[t_start:] and has
    num_inference_steps - t_start steps.  ValueError for a strength outside [0, 1] or one that leaves no step."""
    if not 0.0 <= strength <= 1.0:
        raise ValueError(f"The value of strength should in [0.0, 1.0] but is {strength}")
    n = int(num_inference_steps)
    t_start = int(max(n - min(n * strength, n), 0))
    if n - t_start < 1:
        raise ValueError(f"After adjusting the num_inference_steps by strength parameter: {strength}, the number of pipeline steps is "
                         f"{n - t_start} which is < 1 and not appropriate for this pipeline.")
    return t_start


@dataclass(frozen=True)
class CLIPTextConfig:
    """One CLIPTextModelWithProjection (transformers' CLIPTextConfig names in the comments)."""
    vocab: int = 49408
    hidden: int = 768              # hidden_size; head dim hidden / heads must be 64
    ff: int = 3072                 # intermediate_size
    heads: int = 12
    layers: int = 12
    max_positions: int = 77
    proj_dim: int = 768            # projection_dim
    eos_token_id: int = 2          # 2 (both SD3 checkpoints): pooled row = argmax(ids); else the first ids == eos_token_id
    act: str = "quick_gelu"        # hidden_act: "quick_gelu" (CLIP-L) or "gelu" (CLIP-G)


@dataclass(frozen=True)
class T5Config:
    """The T5EncoderModel of SD3 (T5 v1.1 XXL: gated-gelu feed-forward, no biases, relative-position bias in block 0)."""
    vocab: int = 32128
    d_model: int = 4096
    d_kv: int = 64
    heads: int = 64
    d_ff: int = 10240
    layers: int = 24
    num_buckets: int = 32
    max_distance: int = 128
    eps: float = 1e-6


@dataclass(frozen=True)
class SD3TextConfig:
    clip_l: CLIPTextConfig = CLIPTextConfig()
    clip_g: CLIPTextConfig = CLIPTextConfig(hidden=1280, ff=5120, heads=20, layers=32, proj_dim=1280, act="gelu")
    t5: Optional[T5Config] = T5Config()    # None: no T5 encoder (prompt_embeds is then [B, 77, joint_dim])
    joint_dim: int = 4096                  # row width of prompt_embeds; equals t5.d_model when T5 is present

    @property
    def pooled_dim(self) -> int:
        return self.clip_l.proj_dim + self.clip_g.proj_dim


SD3_MEDIUM_TEXT = SD3TextConfig()
# the smallest shapes that exercise each risk: dh 64 everywhere; CLIP "g" with erf-GELU and an eos id != 2 (the first-match pooling rule);
# T5 with heads * d_kv = 128 != d_model; 64 pad columns behind the 128 + 192 CLIP columns
SD3_TINY_TEXT = SD3TextConfig(
    clip_l=CLIPTextConfig(vocab=100, hidden=128, ff=256, heads=2, layers=3, proj_dim=96, eos_token_id=2, act="quick_gelu"),
    clip_g=CLIPTextConfig(vocab=100, hidden=192, ff=320, heads=3, layers=4, proj_dim=160, eos_token_id=7, act="gelu"),
    t5=T5Config(vocab=100, d_model=384, d_kv=64, heads=2, d_ff=320, layers=2), joint_dim=384)

_CLIP_ACTS = {"quick_gelu": 0, "gelu": 1}


class pd_sd3_clip_config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("vocab", "hidden", "ff", "heads", "layers", "max_positions", "proj_dim", "eos_token_id", "act")]


class pd_sd3_t5_config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("vocab", "d_model", "d_kv", "heads", "d_ff", "layers", "num_buckets", "max_distance")] + \
               [("eps", C.c_float)]


class pd_sd3_text_config(C.Structure):
    _fields_ = [("clip_l", pd_sd3_clip_config), ("clip_g", pd_sd3_clip_config), ("t5", pd_sd3_t5_config), ("joint_dim", C.c_int32),
                ("reserved", C.c_int32 * 3)]


class pd_sd3_text_args(C.Structure):
    _fields_ = [("batch", C.c_int32), ("t5_len", C.c_int32), ("clip_skip", C.c_int32), ("mem", C.c_int32),
                ("ids_clip_l", C.c_void_p), ("ids_clip_g", C.c_void_p), ("ids_t5", C.c_void_p), ("reserved", C.c_int64 * 3)]


@dataclass(frozen=True)
class SD3VaeConfig:
    """diffusers AutoencoderKL as SD3 ships it (vae/config.json): block_out_channels = ch * ch_mult, layers_per_block = num_res_blocks,
    latent_channels = z_channels, use_quant_conv = use_post_quant_conv = False, one mid-block attention head over all channels."""
    ch: int = 128
    ch_mult: Tuple[int, ...] = (1, 2, 4, 4)
    num_res_blocks: int = 2
    z_channels: int = 16
    out_ch: int = 3
    quant_conv: bool = False
    post_quant_conv: bool = False
    scaling_factor: float = 1.5305
    shift_factor: float = 0.0609

    @property
    def downscale(self) -> int:
        return 1 << (len(self.ch_mult) - 1)


SD3_MEDIUM_VAE = SD3VaeConfig()
SD3_TINY_VAE = SD3VaeConfig(ch=32)     # mid-block attention over 128 channels: the flash kernel's small instantiation


class pd_sd3_vae_config(C.Structure):
    _fields_ = [("ch", C.c_int32), ("num_levels", C.c_int32), ("ch_mult", C.c_int32 * E.PD_MAX_LEVELS), ("num_res_blocks", C.c_int32),
                ("z_channels", C.c_int32), ("out_ch", C.c_int32), ("encoder", C.c_int32), ("quant_conv", C.c_int32),
                ("post_quant_conv", C.c_int32), ("scaling_factor", C.c_double), ("shift_factor", C.c_double)]


def _sd3_vres(prefix, cin, cout):
    out = [(prefix + "norm1.weight", (cin,), "gamma"), (prefix + "norm1.bias", (cin,), "beta")]
    out += list(W._conv(prefix + "conv1.", cin, cout, 3))
    out += [(prefix + "norm2.weight", (cout,), "gamma"), (prefix + "norm2.bias", (cout,), "beta")]
    out += list(W._conv(prefix + "conv2.", cout, cout, 3))
    if cin != cout:
        out += list(W._conv(prefix + "conv_shortcut.", cin, cout, 1))
    return out


def _sd3_vmid(prefix, ch):
    out = _sd3_vres(prefix + "resnets.0.", ch, ch)
    a = prefix + "attentions.0."
    out += [(a + "group_norm.weight", (ch,), "gamma"), (a + "group_norm.bias", (ch,), "beta")]
    for n in ("to_q", "to_k", "to_v", "to_out.0"):      # Linear [C, C]: ldm's 1x1 convs q / k / v / proj_out without the trailing 1, 1
        out += [(a + n + ".weight", (ch, ch), "w"), (a + n + ".bias", (ch,), "b")]
    return out + _sd3_vres(prefix + "resnets.1.", ch, ch)


def sd3_vae_spec(cfg: SD3VaeConfig, encoder: bool = True, prefix: str = "vae."):
    """(name, shape, kind) of every VAE tensor under diffusers' AutoencoderKL names (written from its published layout: diffusers is
    absent offline, so the names are UNPINNED): decoder (conv_in, mid_block, up_blocks.{i} in execution order, conv_norm_out, conv_out),
    post_quant_conv if any, then the encoder (conv_in, down_blocks.{i}, mid_block, conv_norm_out, conv_out) and quant_conv if any."""
    nl = len(cfg.ch_mult)
    top = cfg.ch * cfg.ch_mult[-1]
    d = prefix + "decoder."
    out = list(W._conv(d + "conv_in.", cfg.z_channels, top, 3)) + _sd3_vmid(d + "mid_block.", top)
    block_in = top
    for i in range(nl):                                   # up_blocks.{i} is ldm's up.{nl - 1 - i}
        block_out = cfg.ch * cfg.ch_mult[nl - 1 - i]
        for j in range(cfg.num_res_blocks + 1):
            out += _sd3_vres(d + f"up_blocks.{i}.resnets.{j}.", block_in, block_out)
            block_in = block_out
        if i != nl - 1:
            out += list(W._conv(d + f"up_blocks.{i}.upsamplers.0.conv.", block_in, block_in, 3))
    out += [(d + "conv_norm_out.weight", (cfg.ch,), "gamma"), (d + "conv_norm_out.bias", (cfg.ch,), "beta")]
    out += list(W._conv(d + "conv_out.", cfg.ch, cfg.out_ch, 3))
    if cfg.post_quant_conv:
        out += list(W._conv(prefix + "post_quant_conv.", cfg.z_channels, cfg.z_channels, 1))
    if not encoder:
        return out
    e = prefix + "encoder."
    z2 = 2 * cfg.z_channels
    out += list(W._conv(e + "conv_in.", cfg.out_ch, cfg.ch, 3))
    block_in = cfg.ch
    for i, mult in enumerate(cfg.ch_mult):
        for j in range(cfg.num_res_blocks):
            out += _sd3_vres(e + f"down_blocks.{i}.resnets.{j}.", block_in, cfg.ch * mult)
            block_in = cfg.ch * mult
        if i != nl - 1:
            out += list(W._conv(e + f"down_blocks.{i}.downsamplers.0.conv.", block_in, block_in, 3))
    out += _sd3_vmid(e + "mid_block.", block_in)
    out += [(e + "conv_norm_out.weight", (block_in,), "gamma"), (e + "conv_norm_out.bias", (block_in,), "beta")]
    out += list(W._conv(e + "conv_out.", block_in, z2, 3))
    if cfg.quant_conv:
        out += list(W._conv(prefix + "quant_conv.", z2, z2, 1))
    return out


def synth_sd3_vae_state_dict(cfg: SD3VaeConfig, seed: int = 1234, encoder: bool = True) -> Dict[str, np.ndarray]:
    """Deterministic NumPy weights in the style of weights.synth_vae_state_dict."""
    return {n: W.synth_tensor(n, s, k, seed) for n, s, k in sd3_vae_spec(cfg, encoder)}


def sd3_text_spec(cfg: SD3TextConfig):
    """(name, shape, kind) of every text-encoder tensor under the SD3 checkpoint's names: text_encoder. (CLIP-L), text_encoder_2. (CLIP-G),
    text_encoder_3. (T5; the tied encoder.embed_tokens.weight is not listed)."""
    out = []
    for prefix, c in (("text_encoder.", cfg.clip_l), ("text_encoder_2.", cfg.clip_g)):
        if c is None or c.layers == 0:
            continue
        out += W.clip_text_spec(prefix + "text_model.", c.vocab, c.max_positions, c.hidden, c.ff, c.layers)
        out.append((prefix + "text_projection.weight", (c.proj_dim, c.hidden), "w"))
    t = cfg.t5
    if t is not None and t.layers > 0:
        P, D, I, F = "text_encoder_3.", t.d_model, t.heads * t.d_kv, t.d_ff
        out.append((P + "shared.weight", (t.vocab, D), "w"))
        for i in range(t.layers):
            Bp = f"{P}encoder.block.{i}."
            for nm in ("q", "k", "v"):
                out.append((Bp + f"layer.0.SelfAttention.{nm}.weight", (I, D), "w"))
            out.append((Bp + "layer.0.SelfAttention.o.weight", (D, I), "w"))
            if i == 0:
                out.append((Bp + "layer.0.SelfAttention.relative_attention_bias.weight", (t.num_buckets, t.heads), "w"))
            out.append((Bp + "layer.0.layer_norm.weight", (D,), "gamma"))
            out += [(Bp + "layer.1.DenseReluDense.wi_0.weight", (F, D), "w"), (Bp + "layer.1.DenseReluDense.wi_1.weight", (F, D), "w"),
                    (Bp + "layer.1.DenseReluDense.wo.weight", (D, F), "w")]
            out.append((Bp + "layer.1.layer_norm.weight", (D,), "gamma"))
        out.append((P + "encoder.final_layer_norm.weight", (D,), "gamma"))
    return out


def synth_sd3_text_state_dict(cfg: SD3TextConfig, seed: int = 1234) -> Dict[str, np.ndarray]:
    """Deterministic NumPy weights in the style of weights.synth_text_state_dict (w: N(0, 1 / fan_in), b: N(0, 0.02^2), gamma: 1 + N(0, 0.1^2),
    beta: N(0, 0.1^2)).  T5 has no dh^-0.5 in its attention: like its own initialisation the query projection carries it (x d_kv^-0.5), and the
    token embedding is N(0, 1)."""
    sd = {}
    for n, s, k in sd3_text_spec(cfg):
        a = W.synth_tensor(n, s, k, seed)
        if n.endswith("SelfAttention.q.weight"):
            a = a * np.float32(cfg.t5.d_kv ** -0.5)
        elif n == "text_encoder_3.shared.weight":
            a = a * np.float32(math.sqrt(s[1]))
        sd[n] = a
    return sd


def synth_sd3_token_ids(cfg: SD3TextConfig, batch: int, t5_len: int = 20, seed: int = 7):
    """Synthetic (ids_l, ids_g, ids_t5), int32.  CLIP rows: BOS, a run of random tokens, EOS padding (as CLIPTokenizer pads); CLIP-L's EOS is
    the largest id (the argmax rule), CLIP-G's is its eos_token_id, which no other token takes.  T5 rows: random tokens, 1 (</s>), 0 padding."""
    g = np.random.default_rng(seed)
    out = []
    for c in (cfg.clip_l, cfg.clip_g):
        argmax = c.eos_token_id == 2
        eos = c.vocab - 1 if argmax else c.eos_token_id
        ids = np.full((batch, c.max_positions), eos, np.int32)
        ids[:, 0] = c.vocab - 2
        for b in range(batch):
            n = int(g.integers(3, c.max_positions - 4))
            body = g.integers(8, c.vocab - 2, n)
            ids[b, 1:1 + n] = body
        out.append(ids)
    t = cfg.t5
    if t is None:
        out.append(None)
    else:
        ids = np.zeros((batch, t5_len), np.int32)
        for b in range(batch):
            n = int(g.integers(1, max(2, t5_len - 1)))
            ids[b, :n] = g.integers(2, t.vocab, n)
            ids[b, n] = 1
        out.append(ids)
    return tuple(out)


def t5_relative_buckets(length: int, num_buckets: int = 32, max_distance: int = 128, lib_path: Optional[str] = None) -> np.ndarray:
    """T5Attention._relative_position_bucket (bidirectional) for the relative positions -(length - 1) .. length - 1, as the engine's host
    function computes them (pd_t5_relative_buckets; no GPU involved)."""
    lib = E.load_library(lib_path)
    lib.pd_t5_relative_buckets.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    out = np.empty(2 * length - 1, np.int32)
    if lib.pd_t5_relative_buckets(length, num_buckets, max_distance, out.ctypes.data):
        raise E.PdError(lib.pd_last_error().decode(errors="replace"))
    return out


def flow_match_sigmas(steps: int, shift: float = 3.0, num_train_timesteps: int = 1000) -> np.ndarray:
    """FlowMatchEulerDiscreteScheduler.set_timesteps(num_inference_steps) of the scheduler the reference pipeline holds
    (promptdiffusioncontrolnetpipeline_sd3.py:1086-1088): sigmas[steps + 1], descending, last 0; timestep_i = 1000 sigma_i."""
    shifted = lambda s: shift * s / (1.0 + (shift - 1.0) * s)
    ts = np.linspace(shifted(1.0) * num_train_timesteps, shifted(1.0 / num_train_timesteps) * num_train_timesteps, steps)
    return np.concatenate([shifted(ts / num_train_timesteps), [0.0]]).astype(np.float32)


def sincos_pos_embed(dim: int, grid: int, base_size: int, interpolation_scale: float = 1.0) -> np.ndarray:
    """The 2-D sin/cos table PatchEmbed registers as `pos_embed` ([grid * grid, dim]; first half of the channels encodes the
    column, second half the row) -- real checkpoints carry it as a tensor; this is for synthetic weights."""
    def axis(pos, d):
        omega = 1.0 / 10000 ** (np.arange(d // 2, dtype=np.float64) / (d / 2.0))
        ang = pos.reshape(-1)[:, None] * omega[None]
        return np.concatenate([np.sin(ang), np.cos(ang)], axis=1)
    g = np.arange(grid, dtype=np.float64) / (grid / base_size) / interpolation_scale
    col, row = np.meshgrid(g, g)
    return np.concatenate([axis(col, dim // 2), axis(row, dim // 2)], axis=1).astype(np.float32)


def sd3_param_shapes(cfg: SD3Config) -> Dict[str, tuple]:
    """diffusers state-dict names and shapes of both networks ("transformer." / "controlnet." prefixes)."""
    D, out = cfg.hidden, {}

    def lin(name, n, k):
        out[name + ".weight"], out[name + ".bias"] = (n, k), (n,)

    for net, layers, cn in (("transformer.", cfg.layers, False), ("controlnet.", cfg.cn_layers, True)):
        if layers == 0:
            continue
        pm = cfg.cn_pos_embed_max_size if cn and cfg.cn_pos_embed_max_size else cfg.pos_embed_max_size
        out[net + "pos_embed.proj.weight"], out[net + "pos_embed.proj.bias"] = (D, cfg.in_channels, cfg.patch, cfg.patch), (D,)
        out[net + "pos_embed.pos_embed"] = (1, pm * pm, D)
        if cn:
            out[net + "pos_embed_input.proj.weight"] = (D, cfg.in_channels, cfg.patch, cfg.patch)
            out[net + "pos_embed_input.proj.bias"] = (D,)
            out[net + "down_proj.weight"], out[net + "down_proj.bias"] = (3, 6, 3, 3), (3,)      # promptdiffusioncontrolnet_sd3.py:114
        lin(net + "time_text_embed.timestep_embedder.linear_1", D, 256)
        lin(net + "time_text_embed.timestep_embedder.linear_2", D, D)
        lin(net + "time_text_embed.text_embedder.linear_1", D, cfg.pooled_dim)
        lin(net + "time_text_embed.text_embedder.linear_2", D, D)
        single = cn and cfg.cn_single_blocks
        if not single:
            lin(net + "context_embedder", D, cfg.joint_dim)
        for i in range(layers):
            b = f"{net}transformer_blocks.{i}."
            pre_only = (not cn) and i == layers - 1
            dual = (not single) and i in tuple(cfg.cn_dual_attention_layers if cn else cfg.dual_attention_layers)
            lin(b + "norm1.linear", (9 if dual else 6) * D, D)
            if not single:
                lin(b + "norm1_context.linear", (2 if pre_only else 6) * D, D)
            for n in ("to_q", "to_k", "to_v", "to_out.0") + (() if single else ("add_q_proj", "add_k_proj", "add_v_proj")):
                lin(b + "attn." + n, D, D)
            if cfg.qk_norm:
                for n in ("norm_q", "norm_k") + (() if single else ("norm_added_q", "norm_added_k")):
                    out[b + "attn." + n + ".weight"] = (cfg.head_dim,)
            if dual:
                for n in ("to_q", "to_k", "to_v", "to_out.0"):
                    lin(b + "attn2." + n, D, D)
                if cfg.qk_norm:
                    out[b + "attn2.norm_q.weight"], out[b + "attn2.norm_k.weight"] = (cfg.head_dim,), (cfg.head_dim,)
            lin(b + "ff.net.0.proj", 4 * D, D)
            lin(b + "ff.net.2", D, 4 * D)
            if not pre_only and not single:
                lin(b + "attn.to_add_out", D, D)
                lin(b + "ff_context.net.0.proj", 4 * D, D)
                lin(b + "ff_context.net.2", D, 4 * D)
            if cn:
                lin(f"{net}controlnet_blocks.{i}", D, D)
        if not cn:
            lin(net + "norm_out.linear", 2 * D, D)
            lin(net + "proj_out", cfg.patch * cfg.patch * cfg.out_channels, D)
    return out


def synth_sd3_state_dict(cfg: SD3Config, seed: int = 0) -> Dict[str, np.ndarray]:
    """Deterministic non-degenerate weights (the zero-initialised modules get small non-zero values so that every branch
    contributes); pos_embed.pos_embed is the real sin/cos table."""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, shp in sd3_param_shapes(cfg).items():
        if name.endswith("pos_embed.pos_embed"):
            m = int(round(math.sqrt(shp[1])))
            sd[name] = sincos_pos_embed(shp[2], m, base_size=max(1, m // 2))[None].astype(np.float32)
        elif name.endswith(".bias"):
            sd[name] = (0.05 * rng.standard_normal(shp)).astype(np.float32)
        elif len(shp) == 1:                                   # RMSNorm weights of qk_norm
            sd[name] = (1.0 + 0.1 * rng.standard_normal(shp)).astype(np.float32)
        else:
            fan_in = int(np.prod(shp[1:]))
            scale = 0.5 if "norm1" in name or "norm_out" in name else 1.0     # keep the modulation gates moderate
            sd[name] = (scale * rng.standard_normal(shp) / math.sqrt(fan_in)).astype(np.float32)
    return sd


class SD3Engine:
    """The SD3 networks on one engine (one GPU, one stream).  NumPy arrays or CUDA torch tensors in, the same kind out."""

    def __init__(self, cfg: SD3Config = SD3_MEDIUM, device: int = 0, precision: str = "f16", stream_f32: bool = False,
                 lib_path: Optional[str] = None, fp8: bool = False):
        """fp8 (2-byte modes; BASELINE config #5 "fp8 MFMA"): the projections fed by an AdaLN output -- q/k/v of both
        streams and ff / ff_context net.0 -- take e4m3 operands with one scale per token and per output channel and run on
        the block-scaled K = 128 MFMA (twice the f16 rate); level 2 (= True) also the feed-forward-out projections, whose
        input (the GELU output) is stored as e4m3 under a norm bound.  fp8=1: the first group only.  Everything else stays
        in `precision`."""
        if cfg.qk_norm not in (None, "rms_norm"):
            raise NotImplementedError(f"qk_norm={cfg.qk_norm!r}: only None and 'rms_norm' are built (promptdiffusioncontrolnet_sd3.py:105)")
        for lst, n in ((cfg.dual_attention_layers, cfg.layers), (cfg.cn_dual_attention_layers, cfg.cn_layers)):
            if any(i < 0 or i >= min(n, 32) for i in lst):
                raise ValueError("dual_attention_layers index out of range")
        if cfg.cn_single_blocks and tuple(cfg.cn_dual_attention_layers):
            raise ValueError("SD3SingleTransformerBlock has no second attention: cn_dual_attention_layers must be empty with cn_single_blocks")
        if cfg.layers - 1 in tuple(cfg.dual_attention_layers):
            raise NotImplementedError("the context_pre_only last block cannot carry a second attention")
        self.cfg = cfg
        self.base = E.Engine(W.TINY, device=device, precision=precision, stream_f32=stream_f32, lib_path=lib_path)
        lib = self.base.lib
        lib.pd_sd3_configure.argtypes = [C.c_void_p, C.POINTER(pd_sd3_config)]
        lib.pd_sd3_weights_missing.argtypes = [C.c_void_p]
        lib.pd_sd3_forward.argtypes = [C.c_void_p, C.POINTER(pd_sd3_args), C.c_void_p]
        lib.pd_sd3_control.argtypes = [C.c_void_p, C.POINTER(pd_sd3_args), C.c_int32, C.c_void_p]
        lib.pd_sd3_sample.argtypes = [C.c_void_p, C.POINTER(pd_sd3_args), C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]
        lib.pd_sd3_sample_ex.argtypes = [C.c_void_p, C.POINTER(pd_sd3_args), C.POINTER(pd_sd3_loop_args), C.c_void_p, C.c_int32, C.c_float,
                                         C.c_void_p, C.c_void_p]
        lib.pd_sd3_down_proj.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        lib.pd_sd3_text_configure.argtypes = [C.c_void_p, C.POINTER(pd_sd3_text_config)]
        lib.pd_sd3_text_weights_missing.argtypes = [C.c_void_p]
        lib.pd_sd3_encode_prompt.argtypes = [C.c_void_p, C.POINTER(pd_sd3_text_args), C.c_void_p, C.c_void_p]
        lib.pd_sd3_text_encoder.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        lib.pd_sd3_vae_configure.argtypes = [C.c_void_p, C.POINTER(pd_sd3_vae_config)]
        lib.pd_sd3_vae_weights_missing.argtypes = [C.c_void_p]
        lib.pd_sd3_vae_decode.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p]
        lib.pd_sd3_vae_encode.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p, C.c_int32, C.c_void_p]
        self.text_cfg: Optional[SD3TextConfig] = None
        self.vae_cfg: Optional[SD3VaeConfig] = None
        self.vae_has_encoder = False
        c = pd_sd3_config(cfg.in_channels, cfg.out_channels, cfg.patch, cfg.heads, cfg.head_dim, cfg.layers, cfg.cn_layers,
                          cfg.joint_dim, cfg.pooled_dim, cfg.pos_embed_max_size, cfg.cn_pos_embed_max_size,
                          1 if cfg.force_zeros_for_pooled_projection else 0, 1 if cfg.qk_norm else 0,
                          sum(1 << i for i in cfg.dual_attention_layers), sum(1 << i for i in cfg.cn_dual_attention_layers),
                          1 if cfg.cn_single_blocks else 0)
        self.base._check(lib.pd_sd3_configure(self.base._h, C.byref(c)))
        self.fp8 = 2 if fp8 is True else int(fp8)
        if self.fp8:
            if precision in ("f32", "f16x2"):
                raise ValueError("fp8 needs a 2-byte engine precision (f16 / bf16)")
            self.base.set_option("sd3_fp8", self.fp8)

    def close(self):
        self.base.close()

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd, strict: bool = True) -> None:
        known = {n for n, _ in self.base.param_names()}
        unexpected = []
        for name, arr in (sd.items() if isinstance(sd, dict) else sd):
            if not name.startswith(("transformer.", "controlnet.", "text_encoder.", "text_encoder_2.", "text_encoder_3.", "vae.")):
                continue
            if name.startswith("vae.") and (self.vae_cfg is None or name not in known):
                continue   # no VAE on this engine, or its encoder half was not configured: not its tensors
            if name.startswith("text_encoder"):
                # encoders this engine has not configured, and T5's tied copy of shared.weight, are not its tensors
                if self.text_cfg is None or name == "text_encoder_3.encoder.embed_tokens.weight" or name not in known:
                    continue
            if name in known:
                self.base.load_tensor(name, arr)
            else:
                unexpected.append(name)   # e.g. attn.norm_q / attn2.* of an SD3.5 checkpoint: a different network
        if strict and unexpected:
            raise E.PdError(f"{len(unexpected)} unexpected SD3 tensors (first: {unexpected[0]}): the checkpoint describes blocks "
                            "this engine does not implement (qk_norm / dual_attention_layers?)")
        if strict and self.weights_missing():
            raise E.PdError(f"{self.weights_missing()} SD3 tensors missing after load_state_dict")

    # ------------------------------------------------------------------ text encoders
    # ------------------------------------------------------------------ adapters (pd_lora_*): the base engine's registry holds the SD3 tensors
    def lora_add(self, adapter: int, name: str, up, down, alpha: Optional[float] = None) -> None:
        self.base.lora_add(adapter, name, up, down, alpha=alpha)

    def lora_add_ex(self, adapter: int, name: str, kind: str, up, down, up2=None, down2=None, scale: float = 1.0, magnitude=None) -> None:
        self.base.lora_add_ex(adapter, name, kind, up, down, up2=up2, down2=down2, scale=scale, magnitude=magnitude)

    def lora_set_scales(self, scales) -> None:
        self.base.lora_set_scales(scales)

    def lora_remove(self, adapter: int = -1) -> None:
        self.base.lora_remove(adapter)

    def read_weight(self, name: str) -> np.ndarray:
        """One tensor back under its state-dict name as float32, adapters merged (pd_read_weights)."""
        return self.base.read_weight(name)

    def configure_text(self, cfg: SD3TextConfig = SD3_MEDIUM_TEXT) -> None:
        """Registers CLIP-L, CLIP-G and (unless cfg.t5 is None) the T5 encoder on this engine; their tensors then load through
        load_state_dict under the checkpoint's text_encoder. / text_encoder_2. / text_encoder_3. names.  Once per engine."""
        if cfg.joint_dim != self.cfg.joint_dim or cfg.pooled_dim != self.cfg.pooled_dim:
            raise ValueError(f"text encoders give joint_dim {cfg.joint_dim} / pooled_dim {cfg.pooled_dim}, the SD3 networks take "
                             f"{self.cfg.joint_dim} / {self.cfg.pooled_dim}")
        for c in (cfg.clip_l, cfg.clip_g):
            if c.act not in _CLIP_ACTS:
                raise ValueError(f"CLIP hidden_act {c.act!r}: only {sorted(_CLIP_ACTS)} are built")
        c = pd_sd3_text_config()
        for dst, src in ((c.clip_l, cfg.clip_l), (c.clip_g, cfg.clip_g)):
            (dst.vocab, dst.hidden, dst.ff, dst.heads, dst.layers, dst.max_positions, dst.proj_dim, dst.eos_token_id, dst.act) = (
                src.vocab, src.hidden, src.ff, src.heads, src.layers, src.max_positions, src.proj_dim, src.eos_token_id, _CLIP_ACTS[src.act])
        if cfg.t5 is not None:
            t = cfg.t5
            (c.t5.vocab, c.t5.d_model, c.t5.d_kv, c.t5.heads, c.t5.d_ff, c.t5.layers, c.t5.num_buckets, c.t5.max_distance, c.t5.eps) = (
                t.vocab, t.d_model, t.d_kv, t.heads, t.d_ff, t.layers, t.num_buckets, t.max_distance, t.eps)
        c.joint_dim = cfg.joint_dim
        self.base._check(self.base.lib.pd_sd3_text_configure(self.base._h, C.byref(c)))
        self.base._shapes = None      # (the registry grew: read_weight / lora_add_ex look names up again)
        self.text_cfg = cfg

    def text_weights_missing(self) -> int:
        return int(self.base.lib.pd_sd3_text_weights_missing(self.base._h))

    def _ids(self, ids, length, what):
        """int32 [B, length] ids as (owner, pointer, mem)."""
        if E._is_torch(ids):
            import torch
            t = ids.detach().to(torch.int32).contiguous()
            if t.is_cuda:
                if t.ndim != 2 or (length and t.shape[1] != length):
                    raise ValueError(f"{what} must be [B, {length or 'L'}]")
                return t, t.data_ptr(), E.PD_MEM_DEVICE
            ids = t.numpy()
        a = np.ascontiguousarray(ids, np.int32)
        if a.ndim != 2 or (length and a.shape[1] != length):
            raise ValueError(f"{what} must be [B, {length or 'L'}]")
        return a, a.ctypes.data, E.PD_MEM_HOST

    def encode_prompt_ids(self, ids_l, ids_g, ids_t5=None, clip_skip: Optional[int] = None, zero_t5_rows: bool = False):
        """encode_prompt after tokenisation (promptdiffusioncontrolnetpipeline_sd3.py:443-471): token ids [B, 77] x 2 and [B, Lt] ->
        (prompt_embeds [B, 77 + Lt, joint_dim], pooled [B, pooled_dim]), fp32; NumPy in, NumPy out, CUDA torch in, CUDA torch out.
        clip_skip None = 0: hidden_states[-2].  Without a T5 encoder the result is [B, 77, joint_dim]; zero_t5_rows appends the
        [B, 77, joint_dim] zero block the reference concatenates in that case."""
        if self.text_cfg is None:
            raise E.PdError("this engine has no text encoders: call configure_text first")
        cfg = self.text_cfg
        has_t5 = cfg.t5 is not None
        if has_t5 and ids_t5 is None:
            raise ValueError("ids_t5 is required: this engine has a T5 encoder")
        keep = [self._ids(ids_l, cfg.clip_l.max_positions, "ids_l"), self._ids(ids_g, cfg.clip_g.max_positions, "ids_g")]
        if has_t5:
            keep.append(self._ids(ids_t5, 0, "ids_t5"))
        mems = {k[2] for k in keep}
        Bn = keep[0][0].shape[0]
        if len(mems) != 1 or any(k[0].shape[0] != Bn for k in keep):
            raise ValueError("all id arrays of one call must share the batch size and the memory space")
        mem = mems.pop()
        Lt = keep[2][0].shape[1] if has_t5 else 0
        if has_t5 and not 1 <= Lt <= 512:
            raise ValueError(f"ids_t5 must hold 1 to 512 tokens per row, got {Lt}")
        a = pd_sd3_text_args()
        a.batch, a.t5_len, a.clip_skip, a.mem = Bn, Lt, int(clip_skip or 0), mem
        a.ids_clip_l, a.ids_clip_g = keep[0][1], keep[1][1]
        a.ids_t5 = keep[2][1] if has_t5 else None
        pe, pe_ptr = self._out(mem, keep[0][0], (Bn, 77 + Lt, cfg.joint_dim))
        po, po_ptr = self._out(mem, keep[0][0], (Bn, cfg.pooled_dim))
        self.base._order_after_torch(mem)
        self.base._check(self.base.lib.pd_sd3_encode_prompt(self.base._h, C.byref(a), pe_ptr, po_ptr))
        if zero_t5_rows and not has_t5:
            if mem == E.PD_MEM_DEVICE:
                import torch
                pe = torch.cat([pe, torch.zeros_like(pe)], 1)
            else:
                pe = np.concatenate([pe, np.zeros_like(pe)], 1)
        return pe, po

    def text_encoder(self, which: str, ids, clip_skip: Optional[int] = None):
        """One encoder alone.  which "clip_l" / "clip_g": ids [B, 77] -> (hidden_states[-(clip_skip + 2)] [B, 77, hidden], text_embeds
        [B, proj_dim]); "t5": ids [B, Lt] -> last_hidden_state [B, Lt, d_model]."""
        if self.text_cfg is None:
            raise E.PdError("this engine has no text encoders: call configure_text first")
        idx = {"clip_l": 0, "clip_g": 1, "t5": 2}[which]
        if idx == 2:
            if self.text_cfg.t5 is None:
                raise E.PdError("this engine has no T5 encoder")
            owner, ptr, mem = self._ids(ids, 0, "ids")
            Bn, L = owner.shape
            out, optr = self._out(mem, owner, (Bn, L, self.text_cfg.t5.d_model))
            self.base._order_after_torch(mem)
            self.base._check(self.base.lib.pd_sd3_text_encoder(self.base._h, 2, ptr, Bn, L, 0, mem, optr, None))
            return out
        c = (self.text_cfg.clip_l, self.text_cfg.clip_g)[idx]
        owner, ptr, mem = self._ids(ids, c.max_positions, "ids")
        Bn = owner.shape[0]
        hid, hptr = self._out(mem, owner, (Bn, c.max_positions, c.hidden))
        po, pptr = self._out(mem, owner, (Bn, c.proj_dim))
        self.base._order_after_torch(mem)
        self.base._check(self.base.lib.pd_sd3_text_encoder(self.base._h, idx, ptr, Bn, c.max_positions, int(clip_skip or 0), mem, hptr, pptr))
        return hid, po

    # ------------------------------------------------------------------ VAE
    def configure_vae(self, cfg: SD3VaeConfig = SD3_MEDIUM_VAE, encoder: bool = True) -> None:
        """Registers SD3's VAE (decoder, and the encoder unless encoder=False) on this engine; its tensors then load through
        load_state_dict under the checkpoint's ``vae.`` names.  Once per engine."""
        if len(cfg.ch_mult) > E.PD_MAX_LEVELS:
            raise ValueError(f"at most {E.PD_MAX_LEVELS} levels")
        if cfg.z_channels != self.cfg.in_channels:
            raise ValueError(f"the VAE has {cfg.z_channels} latent channels, the SD3 networks take {self.cfg.in_channels}")
        c = pd_sd3_vae_config()
        c.ch, c.num_levels, c.num_res_blocks, c.z_channels, c.out_ch = cfg.ch, len(cfg.ch_mult), cfg.num_res_blocks, cfg.z_channels, cfg.out_ch
        for i, m in enumerate(cfg.ch_mult):
            c.ch_mult[i] = m
        c.encoder, c.quant_conv, c.post_quant_conv = int(bool(encoder)), int(cfg.quant_conv), int(cfg.post_quant_conv)
        c.scaling_factor, c.shift_factor = float(cfg.scaling_factor), float(cfg.shift_factor)
        self.base._check(self.base.lib.pd_sd3_vae_configure(self.base._h, C.byref(c)))
        self.base._shapes = None      # (the registry grew: read_weight / lora_add_ex look names up again)
        self.vae_cfg, self.vae_has_encoder = cfg, bool(encoder)

    def vae_weights_missing(self) -> int:
        return int(self.base.lib.pd_sd3_vae_weights_missing(self.base._h))

    def _need_vae(self, encoder: bool = False):
        if self.vae_cfg is None or (encoder and not self.vae_has_encoder):
            raise E.PdError("this engine has no SD3 VAE" + (" encoder" if encoder else "") + ": call configure_vae first")
        return self.vae_cfg

    # tiled / sliced VAE calls (pd_vae_set_tiling with PD_VAE_SD3): Engine's four, on this engine's own VAE state
    def set_vae_tiling(self, on: bool = True, tile_latent: Optional[int] = None, overlap_factor: Optional[float] = None,
                       tile_batch: Optional[int] = None) -> None:
        """vae.enable_tiling / disable_tiling for every later vae_decode / vae_encode (encode_support_pair included): latents above
        tile_latent (default 128, 1024 pixels) per side run as overlapping tiles blended over overlap_factor (default 0.25) of a tile.  on=True replaces the three parameters
        (None: the default); on=False keeps what a None stands for."""
        self.base._check(self.base.lib.pd_vae_set_tiling(self.base._h, E.PD_VAE_SD3, int(bool(on)), int(tile_latent or 0),
                                                         float(overlap_factor or 0.0), int(tile_batch or 0)))

    def set_vae_slicing(self, on: bool = True) -> None:
        self.base._check(self.base.lib.pd_vae_set_slicing(self.base._h, E.PD_VAE_SD3, int(bool(on))))

    @property
    def vae_tiling(self) -> "E.VaeTilingState":
        t, s, n, b, f = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_double()
        self.base._check(self.base.lib.pd_vae_get_tiling(self.base._h, E.PD_VAE_SD3, C.byref(t), C.byref(s), C.byref(n), C.byref(f), C.byref(b)))
        return E.VaeTilingState(bool(t.value), bool(s.value), int(n.value), float(f.value), int(b.value))

    def vae_tile_plan(self, h: int, w: int, encode: bool = False) -> "E.VaeTilePlan":
        st = self.vae_tiling
        return E.vae_tile_plan(h, w, st.tile_latent, st.overlap_factor, 8, encode)

    def vae_decode(self, latents, raw: bool = False):
        """vae.decode(latents / scaling_factor + shift_factor) (promptdiffusioncontrolnetpipeline_sd3.py:1271-1273): latents
        [B, z, h, w] -> images [B, 3, 8h, 8w] in about [-1, 1]; raw=True decodes the latents as they are.  NumPy in, NumPy out; CUDA
        tensor in, CUDA tensor out."""
        cfg = self._need_vae()
        b = E._Buf(latents)
        if b.owner.ndim != 4 or b.owner.shape[1] != cfg.z_channels:
            raise ValueError(f"latents must be [B, {cfg.z_channels}, h, w]")
        Bn, _, h, w = b.owner.shape
        out, optr = self._out(b.mem, b.owner, (Bn, cfg.out_ch, cfg.downscale * h, cfg.downscale * w))
        self.base._order_after_torch(b.mem)
        self.base._check(self.base.lib.pd_sd3_vae_decode(self.base._h, b.ptr, Bn, h, w, b.mem, int(bool(raw)), optr))
        return out

    def vae_encode(self, images, mode: str = "sample", noise=None, raw: bool = False):
        """vae.encode(images).latent_dist, then (z - shift_factor) * scaling_factor (promptdiffusioncontrolnetpipeline_sd3.py:1132-1133):
        images [B, 3, H, W] in [-1, 1] ->
          "sample":  mean + std * noise, noise [B, z, H/8, W/8] from the caller or, with noise=None, the engine's seeded draw (set_rng)
          "mean":    the posterior's mode
          "moments": the encoder's (mean ; logvar) [B, 2z, H/8, W/8], unscaled
        raw=True leaves the shift and the scaling to the caller (what encode_support_pair returns)."""
        cfg = self._need_vae(encoder=True)
        if mode not in E.VAE_ENCODE_MODES:
            raise ValueError(f"mode must be one of {sorted(E.VAE_ENCODE_MODES)}")
        what = E.VAE_ENCODE_MODES[mode]
        b, nb = E._Buf(images), E._Buf(noise)
        if nb.mem is not None and nb.mem != b.mem:
            raise E.PdError("images and noise must live in the same memory space")
        if b.owner.ndim != 4 or b.owner.shape[1] != cfg.out_ch:
            raise ValueError(f"images must be [B, {cfg.out_ch}, H, W]")
        Bn, _, H, Wd = b.owner.shape
        ds, z = cfg.downscale, cfg.z_channels
        if H % ds or Wd % ds:
            raise ValueError(f"H and W must be multiples of {ds}")
        if nb.owner is not None and tuple(nb.owner.shape) != (Bn, z, H // ds, Wd // ds):
            raise ValueError(f"noise must be [{Bn}, {z}, {H // ds}, {Wd // ds}]")
        out, optr = self._out(b.mem, b.owner, (Bn, 2 * z if what == E.PD_VAE_MOMENTS else z, H // ds, Wd // ds))
        self.base._order_after_torch(b.mem)
        self.base._check(self.base.lib.pd_sd3_vae_encode(self.base._h, b.ptr, Bn, H, Wd, b.mem, what,
                                                         nb.ptr if what == E.PD_VAE_SAMPLE else None, int(bool(raw)), optr))
        return out

    def init_random_weights(self, seed: int = 1234) -> None:
        self.base.init_random_weights(seed)

    def encode_support_pair(self, cond, gt, vae=None):
        """SD3PromptDiffusionModel.encode_support_pair (promptdiffusioncontrolnet_sd3.py:189-198): down_proj (Conv2d 6 -> 3, 3x3)
        over cat([cond, gt], 1) on the engine; with a `vae` the caller's encoder turns the result into latents
        (``vae.encode(x).latent_dist.sample()``), as the reference does; without one, an engine with a VAE encoder does the same itself
        (``vae_encode(x, raw=True)``: scaling stays with the caller, as in the reference); an engine without returns the projection."""
        out = self.down_proj(cond, gt)
        if vae is not None:
            return vae.encode(out).latent_dist.sample()
        if self.vae_cfg is not None and self.vae_has_encoder:
            return self.vae_encode(out, mode="sample", raw=True)
        return out

    def down_proj(self, cond, gt):
        """controlnet.down_proj (Conv2d 6 -> 3, 3x3) over cat([cond, gt], 1): cond, gt [B, 3, H, W] -> [B, 3, H, W]."""
        b0, b1 = E._Buf(cond), E._Buf(gt)
        if b0.mem != b1.mem or tuple(b0.owner.shape) != tuple(b1.owner.shape) or b0.owner.shape[1] != 3:
            raise ValueError("cond and gt must be [B, 3, H, W] in the same memory space")
        Bn, _, H, Wd = b0.owner.shape
        if b0.mem == E.PD_MEM_DEVICE:
            import torch
            pair = torch.cat([b0.owner, b1.owner], 1).contiguous()
            out = torch.empty((Bn, 3, H, Wd), dtype=torch.float32, device=pair.device)
            self.base._order_after_torch(b0.mem)
            self.base._check(self.base.lib.pd_sd3_down_proj(self.base._h, pair.data_ptr(), Bn, H, Wd, b0.mem, out.data_ptr()))
        else:
            pair = np.ascontiguousarray(np.concatenate([b0.owner, b1.owner], 1), np.float32)
            out = np.empty((Bn, 3, H, Wd), np.float32)
            self.base._check(self.base.lib.pd_sd3_down_proj(self.base._h, pair.ctypes.data, Bn, H, Wd, b0.mem, out.ctypes.data))
        return out

    def weights_missing(self) -> int:
        """SD3 tensors still unloaded: both networks, plus the text encoders / the VAE once configure_text / configure_vae registered them."""
        n = int(self.base.lib.pd_sd3_weights_missing(self.base._h))
        n += self.text_weights_missing() if self.text_cfg is not None else 0
        return n + (self.vae_weights_missing() if self.vae_cfg is not None else 0)

    # ------------------------------------------------------------------ calls
    def _args(self, latents, context, pooled, cond, pair, scale, timestep=None, rows=None, cn_pooled=None, like=None):
        """like: the tensor whose shape stands in for `latents` when a seeded or img2img call passes none"""
        bufs = [E._Buf(x) for x in (latents, context, pooled, cond, pair, cn_pooled)]
        mems = {b.mem for b in bufs if b.mem is not None}
        if len(mems) != 1:
            raise ValueError("all tensors of one call must live in the same memory space (NumPy / CPU or one CUDA device)")
        mem = mems.pop()
        lat = bufs[0].owner if bufs[0].owner is not None else like
        B, _, H, Wd = lat.shape
        rows = rows or B
        if tuple(bufs[1].owner.shape[::2]) != (rows, self.cfg.joint_dim) or tuple(bufs[2].owner.shape) != (rows, self.cfg.pooled_dim):
            raise ValueError(f"context must be [{rows}, S, {self.cfg.joint_dim}] and pooled [{rows}, {self.cfg.pooled_dim}]")
        for b in bufs[3:5]:
            if b.owner is not None and tuple(b.owner.shape) != tuple(lat.shape):
                raise ValueError("cond / pair latents must have the shape of latents")
        if bufs[5].owner is not None and tuple(bufs[5].owner.shape) != (rows, self.cfg.pooled_dim):
            raise ValueError(f"controlnet_pooled_projections must be [{rows}, {self.cfg.pooled_dim}]")
        a = pd_sd3_args()
        a.batch, a.height, a.width, a.context_len, a.mem = B, H, Wd, bufs[1].owner.shape[1], mem
        a.conditioning_scale = float(scale)
        a.latents, a.context, a.pooled, a.cond, a.pair, a.cn_pooled = (b.ptr for b in bufs)
        keep = bufs
        if timestep is not None:
            t = np.ascontiguousarray(np.broadcast_to(np.asarray(E._to_host(timestep), np.float32), (B,)))
            a.timestep = t.ctypes.data
            keep = bufs + [t]
        self.base._order_after_torch(mem)
        return a, keep, mem, lat

    def _out(self, mem, like, shape):
        if mem == E.PD_MEM_DEVICE:
            import torch
            o = torch.empty(shape, dtype=torch.float32, device=like.device)
            return o, o.data_ptr()
        o = np.empty(shape, np.float32)
        return o, o.ctypes.data

    def forward(self, latents, timestep, context, pooled, cond=None, pair=None, conditioning_scale: float = 1.0,
                controlnet_pooled_projections=None):
        """One evaluation: transformer(latents, timestep, context, pooled | ControlNet(cond, pair) residuals) -> velocity.
        The ControlNet's pooled projections are zeros under force_zeros_for_pooled_projection (the reference default), else
        `controlnet_pooled_projections`, else `pooled` (pipeline :1164-1168)."""
        a, keep, mem, lat = self._args(latents, context, pooled, cond, pair, conditioning_scale, timestep,
                                       cn_pooled=controlnet_pooled_projections)
        out, ptr = self._out(mem, lat, (a.batch, self.cfg.out_channels, a.height, a.width))
        self.base._check(self.base.lib.pd_sd3_forward(self.base._h, C.byref(a), ptr))
        return out

    def controlnet(self, latents, timestep, context, pooled, cond, pair, conditioning_scale: float = 1.0):
        """SD3PromptDiffusionModel.forward: the list of cn_layers scaled residuals [B, N, hidden].  `pooled` is what the
        ControlNet itself is given (the pipeline passes zeros under force_zeros_for_pooled_projection)."""
        res = []
        for i in range(self.cfg.cn_layers):
            a, keep, mem, lat = self._args(latents, context, pooled, cond, pair, conditioning_scale, timestep, cn_pooled=pooled)
            n = (a.height // self.cfg.patch) * (a.width // self.cfg.patch)
            out, ptr = self._out(mem, lat, (a.batch, n, self.cfg.hidden))
            self.base._check(self.base.lib.pd_sd3_control(self.base._h, C.byref(a), i, ptr))
            res.append(out)
        return res

    def sample(self, latents, prompt_embeds, pooled_prompt_embeds, negative_prompt_embeds=None, negative_pooled_prompt_embeds=None,
               control_latents=None, pair_latents=None, num_inference_steps: int = 28, guidance_scale: float = 7.0,
               controlnet_conditioning_scale: float = 1.0, shift: float = 3.0, sigmas=None, control_guidance_start: float = 0.0,
               control_guidance_end: float = 1.0, controlnet_pooled_projections=None, init_latents=None, mask=None, noise=None,
               from_seed: bool = False):
        """The denoising loop of the reference's __call__ (promptdiffusioncontrolnetpipeline_sd3.py:1192-1245) from initial
        noise `latents` to final latents.  guidance_scale > 1 needs the negative embeddings (batch [negative ; positive]).

        Img2img / inpainting / seeded noise (pd_sd3_sample_ex; arithmetic in include/pdengine.h, pd_sd3_loop_args), on the `sigmas`
        given -- truncating the grid by a strength is the caller's (img2img_start):
          init_latents [B, C, h, w]  z0: the loop starts from sigmas[0] eps + (1 - sigmas[0]) z0, eps = `noise`, else `latents`
          mask [B, 1, h, w] (or [B, h, w])  needs init_latents; after every step x <- (1 - m) k + m x, 1 = repaint
          from_seed                  eps (without init_latents: the start latents) is the engine's draw at ("xt", 0) under set_rng;
                                     `latents` and `noise` must be None
        A call that uses none of the four runs the plain loop exactly as before."""
        edit = init_latents is not None or mask is not None or noise is not None or from_seed
        if edit:
            if mask is not None and init_latents is None:
                raise ValueError("`mask` needs `init_latents`")
            if noise is not None and init_latents is None:
                raise ValueError("`noise` needs `init_latents` (the start latents of a plain call are `latents`)")
            if from_seed and (latents is not None or noise is not None):
                raise ValueError("from_seed draws the noise in the engine: `latents` and `noise` must be None")
            if not from_seed and latents is None and noise is None:
                raise ValueError("the noise is required: `latents`, `noise` or from_seed=True")
            if noise is not None:
                latents = None                       # eps is `noise`; pd_sd3_sample_ex ignores args->latents then
        like = next((t for t in (latents, noise, init_latents, control_latents) if t is not None), None)
        if like is None:
            raise ValueError("from_seed without `init_latents` needs `control_latents` to give the latent shape")
        cfg_on = guidance_scale > 1.0
        if cfg_on and (negative_prompt_embeds is None or negative_pooled_prompt_embeds is None):
            raise ValueError("guidance_scale > 1 needs negative_prompt_embeds and negative_pooled_prompt_embeds")
        if cfg_on:
            if E._is_torch(prompt_embeds):
                import torch
                ctx = torch.cat([negative_prompt_embeds, prompt_embeds], 0)
                pooled = torch.cat([negative_pooled_prompt_embeds, pooled_prompt_embeds], 0)
            else:
                ctx = np.concatenate([negative_prompt_embeds, prompt_embeds], 0)
                pooled = np.concatenate([negative_pooled_prompt_embeds, pooled_prompt_embeds], 0)
        else:
            ctx, pooled = prompt_embeds, pooled_prompt_embeds
        sig = flow_match_sigmas(num_inference_steps, shift) if sigmas is None else np.ascontiguousarray(sigmas, np.float32)
        if sig.shape != (num_inference_steps + 1,):
            raise ValueError("sigmas must hold num_inference_steps + 1 values")
        B = like.shape[0]
        a, keep, mem, lat = self._args(latents, ctx, pooled, control_latents, pair_latents, controlnet_conditioning_scale,
                                       rows=2 * B if cfg_on else B, cn_pooled=controlnet_pooled_projections, like=like)
        loop = None
        if edit:
            if mask is not None and len(mask.shape) == 3:
                mask = mask[:, None]
            extra = [E._Buf(t) for t in (init_latents, mask, noise)]
            for b, shp, what in zip(extra, (tuple(lat.shape), (B, 1) + tuple(lat.shape[2:]), tuple(lat.shape)), ("init_latents", "mask", "noise")):
                if b.owner is None:
                    continue
                if b.mem != mem:
                    raise ValueError("all tensors of one call must live in the same memory space (NumPy / CPU or one CUDA device)")
                if tuple(b.owner.shape) != shp:
                    raise ValueError(f"`{what}` must be {list(shp)}, got {list(b.owner.shape)}")
            keep = keep + extra
            loop = pd_sd3_loop_args()
            loop.init_latents, loop.mask, loop.noise = (b.ptr for b in extra)
            loop.flags = PD_XT_FROM_SEED if from_seed else 0
            self.base._order_after_torch(mem)
        # controlnet_keep (pipeline :1155-1162): the ControlNet acts on the steps inside [start, end] of the schedule
        n = num_inference_steps
        keep_steps = np.array([1.0 - float(i / n < control_guidance_start or (i + 1) / n > control_guidance_end) for i in range(n)],
                              np.float32)
        scales = np.ascontiguousarray(keep_steps * np.float32(controlnet_conditioning_scale))
        out, ptr = self._out(mem, lat, tuple(lat.shape))
        if loop is not None:
            self.base._check(self.base.lib.pd_sd3_sample_ex(self.base._h, C.byref(a), C.byref(loop), sig.ctypes.data, num_inference_steps,
                                                            float(guidance_scale), scales.ctypes.data, ptr))
            return out
        self.base._check(self.base.lib.pd_sd3_sample(self.base._h, C.byref(a), sig.ctypes.data, num_inference_steps,
                                                     float(guidance_scale), scales.ctypes.data, ptr))
        return out

    def set_rng(self, seed: int, sample_base: int = 0) -> None:
        """Seed and first global sample index of the engine's Philox generator (Engine.set_rng): what from_seed and
        vae_encode(mode="sample") without noise draw from."""
        self.base.set_rng(seed, sample_base)

    @property
    def rng(self) -> Tuple[int, int]:
        return self.base.rng

    def randn(self, shape, stream="step", draw: int = 0, device=None):
        """The standard normals the engine draws at (stream, draw) (Engine.randn); from_seed consumes ("xt", 0)."""
        return self.base.randn(shape, stream=stream, draw=draw, device=device)
