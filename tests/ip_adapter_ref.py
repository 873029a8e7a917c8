"""References for the IP-Adapter image term: the fp64 reference and per-element bound of ip_attn_add_kernel (csrc/ip_attention.hip), and a
NumPy restatement of a UNet with decoupled cross-attention built on the oracle.  Pure NumPy on the CPU, no engine import: shared by
test_ip_adapter_cpu.py (the bound has teeth; effect size of the seeded adapter) and test_ip_adapter_gpu.py.

The kernel.  With q, att [B, N, C], K_ip, V_ip [Bk, T, C] as stored in the compute type T and o = attention (tests/attn_ref.py: per head
softmax(scale q K_ip^T) V_ip, the keys of sample 0 for every sample when Bk = 1),
    out = round_T(att + s o)
The kernel computes o in fp32 as the attention kernels do (logits, exp2-based softmax over tiles of 32 keys, fp32 accumulation) and never
rounds it to T; then t1 = fl32(s o'), t2 = fl32(att + t1), out = round_T(t2).  Error of out against the fp64 value, per element:
    |s| attention_bound("f32", q, K_ip, V_ip)    everything inside o', under attn_ref.py's fp32 model in EVERY mode: the kernel widens the
                                                 stored operands to fp32 exactly and from there on has no 2-byte rounding (no operand
                                                 re-rounding, no rounded P, no rounded o), so the 2-byte models' u_q / u_p / u_out |o| terms
                                                 do not apply -- with them a kernel that rounds o to T before the add would pass
    + U32 |s o|                                  the multiply: one fp32 rounding at the magnitude of its result
    + U32 (|att| + |s o|)                        the add: one fp32 rounding, at most the magnitude of its operands
    + u_out |att + s o|                          the store (0 in the fp32-storage modes)
att is an input already held in T: it carries no error of its own.  The three fp32 terms are first order; the factor (1 + u_out) that the
store's relative rounding puts on the errors before it is applied to them as attn_ref.py does.  Unit roundoffs and operation counts
are the only constants.

The restatement.  oracle.pd_oracle.cross_attention is wrapped at run time (ip_active): for the UNet's attn2 layers (Net.prefix tells the
UNet from the ControlNet, which carries no adapter) the image term s_j softmax(q K_ip^T / sqrt(dh)) V_ip is added before to_out."""
import contextlib

import numpy as np

from oracle import pd_oracle as O
from tests import attn_ref as R
from tests.norm_ref import U32, U_OUT

UNET = "model.diffusion_model."
KERNEL_MUTANTS = ("k_next_head", "drop_last", "pad_key", "scale_in_softmax", "round_o", "swap_samples")


# ------------------------------------------------------------------------------------------------ the kernel
def _expand(t, B):
    return np.broadcast_to(t, (B,) + t.shape[1:]) if t.shape[0] == 1 and B > 1 else t


def ip_attn_add_ref(q, att, k, v, heads, s, mode=None, mutant=None):
    """fp64 att + s softmax(q k^T dh^-0.5) v, [B, N, C]; (result, o).  mutant: one of KERNEL_MUTANTS -- next head's keys, last key
    dropped, a zero pad key counted (attn_ref's), s applied to the logits instead of the output, o rounded to the compute type of
    `mode` before the add, the keys and values of the samples rolled by one (what swapping the guidance halves does to a batch)."""
    assert mutant is None or mutant in KERNEL_MUTANTS
    B = q.shape[0]
    k, v = np.ascontiguousarray(_expand(k, B)), np.ascontiguousarray(_expand(v, B))
    if mutant == "swap_samples":
        k, v = np.roll(k, 1, axis=0), np.roll(v, 1, axis=0)
    dh = q.shape[2] // heads
    if mutant == "scale_in_softmax":
        o, _ = R.attention_ref(q, k, v, heads, scale=float(s) * dh ** -0.5)
        return att.astype(np.float64) + o, o
    o, _ = R.attention_ref(q, k, v, heads, mutant=mutant if mutant in R.MUTANTS else None)
    if mutant == "round_o":
        o = R.round_like(o.astype(np.float32), mode).astype(np.float64)
    return att.astype(np.float64) + float(s) * o, o


def ip_attn_add_bound(mode, q, att, k, v, heads, s):
    """The per-element bound of the module docstring, [B, N, C]."""
    B = q.shape[0]
    k, v = np.ascontiguousarray(_expand(k, B)), np.ascontiguousarray(_expand(v, B))
    ref, o = ip_attn_add_ref(q, att, k, v, heads, s)
    u_out = U_OUT[R.STORAGE[mode]]
    so = np.abs(float(s) * o)
    inner = abs(float(s)) * R.attention_bound("f32", q, k, v, heads) + U32 * so + U32 * (np.abs(att.astype(np.float64)) + so)
    return (1 + u_out) * inner + u_out * np.abs(ref)


def make_kernel_inputs(family, seed, B, N, C, heads, T, mode, Bk=None):
    """q, att [B, N, C], k, v [Bk, T, C] of one attn_ref family, rounded to the compute type of `mode`; att ~ N(0, 1)"""
    Bk = B if Bk is None else Bk
    q, k, v = R.make_inputs(family, seed, B, N, T, heads, C // heads, mode)
    att = R.round_like(np.random.default_rng(seed + 17).standard_normal((B, N, C)).astype(np.float32), mode)
    return q, att, np.ascontiguousarray(k[:Bk]), np.ascontiguousarray(v[:Bk])


# ------------------------------------------------------------------------------------------------ the network
def image_tokens(ip_sd, embeds, num_tokens):
    """ImageProjection: LayerNorm(reshape(proj(e), [T, D])), [n, T, D] fp32"""
    e = np.asarray(embeds, np.float32)
    p = O.linear(e, ip_sd["image_proj.proj.weight"], ip_sd["image_proj.proj.bias"])
    p = p.reshape(e.shape[0], num_tokens, -1)
    return O.layer_norm(p, ip_sd["image_proj.norm.weight"], ip_sd["image_proj.norm.bias"])


def _attend(q, k, v, heads):
    B, N, C = q.shape
    dh = C // heads
    sp = lambda t: t.reshape(t.shape[0], t.shape[1], heads, dh).transpose(0, 2, 1, 3)
    q, k, v = sp(q), sp(k), sp(v)
    sim = np.matmul(q, k.transpose(0, 1, 3, 2)) * np.float32(dh ** -0.5)
    sim = sim - sim.max(axis=-1, keepdims=True)
    e = np.exp(sim)
    return np.matmul(e / e.sum(axis=-1, keepdims=True), v).transpose(0, 2, 1, 3).reshape(B, N, C)


@contextlib.contextmanager
def ip_active(ip_sd, slots, tokens, scales):
    """While it lives, oracle.pd_oracle.cross_attention adds the image term in the UNet's attn2 layers.  slots: {SpatialTransformer
    prefix relative to the network ("input_blocks.1.1."): j}; tokens [Bf or 1, T, D] in the batch order of the call (under guidance
    [unconditional ; conditional]); scales: s_j per block."""
    orig = O.cross_attention

    def cross_attention(p, pre, x, context=None, heads=8):
        st = pre[:-len("transformer_blocks.0.attn2.")] if pre.endswith("transformer_blocks.0.attn2.") else None
        if context is None or p.prefix != UNET or st not in slots or float(scales[slots[st]]) == 0.0:
            return orig(p, pre, x, context, heads)
        j = slots[st]
        q = O.linear(x, p(pre + "to_q.weight"))
        out = _attend(q, O.linear(context, p(pre + "to_k.weight")), O.linear(context, p(pre + "to_v.weight")), heads)
        tok = np.broadcast_to(tokens, (q.shape[0],) + tokens.shape[1:]) if tokens.shape[0] == 1 else tokens
        assert tok.shape[0] == q.shape[0], (tok.shape, q.shape)
        kip = O.linear(tok, ip_sd[f"ip_adapter.{2 * j + 1}.to_k_ip.weight"])
        vip = O.linear(tok, ip_sd[f"ip_adapter.{2 * j + 1}.to_v_ip.weight"])
        out = out + np.float32(scales[j]) * _attend(q, kip, vip, heads)
        return O.linear(out, p(pre + "to_out.0.weight"), p(pre + "to_out.0.bias"))

    O.cross_attention = cross_attention
    try:
        yield
    finally:
        O.cross_attention = orig


def slots_of(prefixes):
    """{relative SpatialTransformer prefix: j} from ip_adapter.block_prefixes(cfg, prefix="")"""
    return {p: j for j, p in enumerate(prefixes)}


def call_tokens(ip_sd, num_tokens, cond, uncond, B, use_cfg):
    """The tokens of a network call at sampling batch B: cond / uncond [Bi, E] (uncond None: zeros), Bi = 1 or B."""
    cond = np.asarray(cond, np.float32)
    uncond = np.zeros_like(cond) if uncond is None else np.asarray(uncond, np.float32)
    rep = lambda t: np.repeat(t, B, axis=0) if t.shape[0] == 1 and B > 1 else t
    tc, tu = rep(image_tokens(ip_sd, cond, num_tokens)), rep(image_tokens(ip_sd, uncond, num_tokens))
    return np.concatenate([tu, tc]) if use_cfg else tc
