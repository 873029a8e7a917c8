"""fp64 reference, inputs and a per-element error bound for the attention kernels (attention.hip: attn_kernel, attn2_kernel;
vae_attention.hip).  Pure NumPy / torch on the CPU, no engine import: shared by test_attn_ref_cpu.py (which shows that the bound
has teeth: every mutant of the reference below exceeds it) and test_attention_gpu.py (which holds the HIP kernels to it).

The operation: per (sample b, head h), with q_i, k_k, v_k the dh-wide head slices of the rows, as stored in the compute type T,
    s_ik = scale q_i . k_k + bias_h[k - i + Nk - 1]      (keys k > i masked when causal; bias only for T5)
    p_ik = exp(s_ik - m_i) / l_i,   m_i = max_k s_ik,   l_i = sum_k exp(s_ik - m_i)
    o_id = sum_k p_ik v_kd

Unit roundoffs, and where they come from (u = 2^-p for a format with p significant bits, round to nearest even):
    U32   = 2^-24   fp32: logits, the online softmax, both MFMA accumulators
    bf16  : 2^-8    pd_common.h f2bf / pack2bf (v_cvt_pk_bf16_f32, RNE)         -- the same value as norm_ref.U_FMT / U_OUT
    f16   : 2^-11   pd_common.h f2h / pack2h (v_cvt_f16_f32, RNE)
    f16x2 : 2^-21   pd_mma.h split_f16: an fp32 operand becomes hi = x truncated to fp16 (v_cvt_pkrtz: x - hi is exact and below
                    2^-10 |x|) plus lo = RNE_fp16(x - hi), so |x - hi - lo| <= 2^-11 2^-10 |x|; a lo below fp16's normal range
                    (|x| < 2^-4) keeps an absolute error of half the smallest subnormal instead, 2^-25.  mma<PREC_F16X2> through
                    mma_raw sums all four hi / lo products
    f32   : the fp32 MFMA (v_mfma_f32_16x16x4f32) takes the operands as they are
    output: store4 rounds o to T in the 2-byte modes (norm_ref.U_OUT[T]); the fp32-storage modes store the fp32 value
    exp2  : __builtin_amdgcn_exp2f is v_exp_f32.  No accuracy figure for it is at hand, so it is bounded at one fp32 ulp of its
            result, 2^-23 relative -- a bound, not a measurement.

The error model.  A kernel computes p'_ik = p_ik e^(d_ik) / sum_j p_ij e^(d_ij) with |d_ik| <= theta_ik: everything that perturbs one
logit or one exponential before the row is normalised.  In natural-log units, for the unmasked keys,
    A_ik     = scale sum_d |q_id k_kd|
    theta_ik = u_q A_ik            operand re-rounding: attn2_kernel's SUBM path rescales Q by scale * log2(e) and rounds it to T
                                   again (u_T per element; charged to every 2-byte launch so one bound serves both families); f16x2:
                                   2 * 2^-21, both operands split
             + a_op max(scale, 1) (sum_d |q_id| + sum_d |k_kd|)
                                   the absolute part of those conversions: 2^-25 per element in f16x2 (see above) and in f16 (a
                                   rescaled Q element below fp16's normal range); 0 in bf16, whose exponent range is fp32's
             + (dh + 2) U32 A_ik   fp32 accumulation of the dh products of a logit in any order (sum of n terms: (n - 1) u sum |x|),
                                   one more for SUBM's -m_ref slot, two more for vae_attention.hip's four partial sums
             + 4 U32 (|s_ik| + |bias| + M_i),  M_i = max_k |s_ik|
                                   the exp2 argument: scale * log2(e) is itself rounded, s * sl2, + bias (whose conversion to exp2
                                   units rounds once), - m each round once at the magnitude of their operands; the subtracted
                                   maximum (m, or SUBM's lazily raised m_ref <= (1 + 2^-7) M_i) is at most M_i in magnitude
             + 2^-23               v_exp_f32
Logit errors move numerator and denominator together, so they act on |v_kd - o_id| (o' - o = sum_k (p'_ik - p_ik) (v_kd - o_id)):
    E1_id = e^(2 Theta_i) sum_k p_ik (theta_ik + thetabar_i) |v_kd - o_id|,  thetabar_i = sum_k p_ik theta_ik,  Theta_i = max_k theta_ik
What happens to P after the exponential, with Pv_id = sum_k p_ik |v_kd|:
    E2_id = u_p (Pv_id + |o_id|)   P is rounded to the MFMA operand type (u_T; f16x2: 2^-20 for the splits of P and of V) while the row
                                   sum l is taken from the unrounded P on every path without ONES, so the rounding does not cancel:
                                   it reaches the numerator through |v| and, where l is summed from rounded P (ONES), the denominator
    E3_id = 2 a_p (sum_k |v_kd| + n_i |o_id|) / l_i     (n_i unmasked keys)
                                   fp16 underflow of small P (f16 and the hi / lo halves of f16x2): a P below 2^-14 is a subnormal and
                                   keeps an absolute error of a_p = 2^-25 in the kernel's units, in which the row's largest P is
                                   2^(m_i - m_used) >= 1/2 (m_used is the running maximum of the tiles so far, <= m_i; SUBM's m_ref
                                   sits at most its own rounding above the first tile's maximum) -- hence the factor 2 -- and l_i is
                                   the row sum in units where the largest P is 1.  Negligible unless the row is peaked (l_i near 1)
                                   and long.
           + a_op                  f16x2: the absolute part of V's split, times sum_k p_ik = 1
    E4_id = (n_i + 2 ceil(Nk / 32) + 3) U32 (Pv_id + |o_id|)
                                   fp32 accumulation of the n_i products of o and of the n_i terms of l in any order, one rounding
                                   of each per rescale by alpha (at most one per key tile; the smallest tile is vae_attention.hip's
                                   32; alpha itself multiplies o and l alike and cancels), 1 / l, o * (1 / l)
    bound_id = (1 + u_out) (E1 + E2 + E3 + E4) + u_out |o_id|
Unit roundoffs and operation counts are the only constants: nothing here is fitted to what a kernel returns."""
import numpy as np
import torch

from tests.norm_ref import U32, U_OUT, round_to

LOG2E = 1.4426950408889634
TK = 64                      # keys per tile of attention.hip (the input families place their events relative to it)
LAZY_THR = 8.0               # attn2_kernel's SUBM path raises its reference when a tile exceeds it by more than this (exp2 units)
STORAGE = {"f32": "f32", "f16x2": "f32", "f16": "f16", "bf16": "bf16"}      # the compute type T the kernels read and write
#            u_q        a_op       u_p        a_p
MODEL = {"f32":   (0.0,       0.0,       0.0,       0.0),
         "f16x2": (2.0 ** -20, 2.0 ** -25, 2.0 ** -20, 2.0 ** -25),
         "f16":   (2.0 ** -11, 2.0 ** -25, 2.0 ** -11, 2.0 ** -25),
         "bf16":  (2.0 ** -8,  0.0,       2.0 ** -8,  0.0)}
U_EXP2 = 2.0 ** -23


def round_like(x, mode):
    """x (fp32) as the engine of `mode` holds it in its compute type"""
    return round_to(np.asarray(x, np.float32), STORAGE[mode])


# ------------------------------------------------------------------------------------------------ reference (fp64)
def _heads(t, heads):
    B, N, C = t.shape
    return t.astype(np.float64).reshape(B, N, heads, C // heads).transpose(0, 2, 1, 3)


def _bias_matrix(relbias, h, Nq, Nk, shift=0):
    """bias[i, k] = relbias[h][k - i + Nk - 1 + shift] (index clipped: only the off-by-one mutant leaves the range)"""
    idx = np.arange(Nk)[None, :] - np.arange(Nq)[:, None] + Nk - 1 + shift
    return np.asarray(relbias, np.float64)[h][np.clip(idx, 0, 2 * Nk - 2)]


MUTANTS = ("drop_last", "pad_key", "causal_off1", "bias_off1", "bias_next_head", "k_next_head", "no_log2e", "v_swap", "stale_alpha")


def attention_ref(q, k, v, heads, scale=None, causal=False, relbias=None, mutant=None, want_logits=False):
    """fp64 multi-head attention of q [B, Nq, C], k, v [B, Nk, C] (already rounded to the compute type); relbias [heads, 2 Nk - 1] in
    natural-log units.  Returns (o [B, Nq, C], p [B, heads, Nq, Nk]) and, with want_logits, the masked logits s as a third value.
    mutant: one of MUTANTS -- the mistakes a kernel could make, for test_attn_ref_cpu.py."""
    assert mutant is None or mutant in MUTANTS
    B, Nq, C = q.shape
    Nk = k.shape[1]
    dh = C // heads
    scale = dh ** -0.5 if not scale else float(scale)
    qh, kh, vh = _heads(q, heads), _heads(k, heads), _heads(v, heads)
    o = np.empty((B, heads, Nq, dh))
    P = np.empty((B, heads, Nq, Nk))
    S = np.empty((B, heads, Nq, Nk)) if want_logits else None
    iq, ik = np.arange(Nq)[:, None], np.arange(Nk)[None, :]
    for b in range(B):
        for h in range(heads):
            kk = kh[b, (h + 1) % heads] if mutant == "k_next_head" else kh[b, h]
            s = (qh[b, h] @ kk.T) * scale
            if mutant == "no_log2e":           # exp2(s scale) where exp2(s scale log2 e) was meant
                s = s / LOG2E
            if relbias is not None:
                s = s + _bias_matrix(relbias, (h + 1) % heads if mutant == "bias_next_head" else h, Nq, Nk, 1 if mutant == "bias_off1" else 0)
            if causal:
                s = np.where(ik >= np.maximum(iq, 1) if mutant == "causal_off1" else ik > iq, -np.inf, s)
            if mutant == "drop_last":
                s = s.copy(); s[:, -1] = -np.inf
            vv = vh[b, h]
            if mutant == "pad_key":            # one pad key of the ragged tile, logit 0 and value 0, counted
                s = np.concatenate([s, np.zeros((Nq, 1))], 1)
                vv = np.concatenate([vv, np.zeros((1, dh))], 0)
            if mutant == "v_swap":             # the last key and the first one of its 32-key group swapped on the V side
                c = Nk - 1
                a = c // 32 * 32 if c % 32 else c - 1
                vv = vv.copy(); vv[[a, c]] = vv[[c, a]]
            m = s.max(1, keepdims=True)
            e = np.exp(s - m)
            l = e.sum(1, keepdims=True)
            if mutant == "stale_alpha":        # the accumulator keeps the weights of the running maximum of its own tile
                run = np.maximum.accumulate(np.stack([s[:, t:t + TK].max(1) for t in range(0, s.shape[1], TK)], 1), 1)
                e = np.exp(s - np.repeat(run, TK, 1)[:, :s.shape[1]])
            p = e / l
            o[b, h] = p @ vv
            P[b, h] = p[:, :Nk]
            if want_logits:
                S[b, h] = s[:, :Nk]
    o = o.transpose(0, 2, 1, 3).reshape(B, Nq, C)
    return (o, P, S) if want_logits else (o, P)


# ------------------------------------------------------------------------------------------------ bound
def _dev_sum(w, v, o, chunk=1 << 24):
    """sum_k w[i, k] |v[k, d] - o[i, d]| without holding [Nq, Nk, dh] at once (torch: threaded)"""
    w, v, o = torch.from_numpy(w), torch.from_numpy(v), torch.from_numpy(o)
    out = torch.empty_like(o)
    step = max(1, chunk // (v.shape[0] * v.shape[1]))
    for i in range(0, o.shape[0], step):
        out[i:i + step] = ((v[None] - o[i:i + step, None]).abs_() * w[i:i + step, :, None]).sum(1)
    return out.numpy()


def attention_bound(mode, q, k, v, heads, scale=None, causal=False, relbias=None):
    """The per-element bound of the module docstring, [B, Nq, C]."""
    u_q, a_op, u_p, a_p = MODEL[mode]
    u_out = U_OUT[STORAGE[mode]]
    B, Nq, C = q.shape
    Nk = k.shape[1]
    dh = C // heads
    scale = dh ** -0.5 if not scale else float(scale)
    qh, kh, vh = _heads(q, heads), _heads(k, heads), _heads(v, heads)
    out = np.empty((B, heads, Nq, dh))
    iq, ik = np.arange(Nq)[:, None], np.arange(Nk)[None, :]
    live = ik <= iq if causal else np.ones((Nq, Nk), bool)
    n_i = live.sum(1, keepdims=True).astype(np.float64)
    for b in range(B):
        for h in range(heads):
            qq, kk, vv = qh[b, h], kh[b, h], vh[b, h]
            dot = (qq @ kk.T) * scale
            bias = _bias_matrix(relbias, h, Nq, Nk) if relbias is not None else 0.0
            s = np.where(live, dot + bias, -np.inf)
            m = s.max(1, keepdims=True)
            e = np.exp(s - m)
            l = e.sum(1, keepdims=True)
            p = e / l
            o = p @ vv
            A = (np.abs(qq) @ np.abs(kk).T) * scale
            M = np.abs(np.where(live, s, 0.0)).max(1, keepdims=True)
            theta = (u_q + (dh + 2) * U32) * A + a_op * max(scale, 1.0) * (np.abs(qq).sum(1)[:, None] + np.abs(kk).sum(1)[None, :]) \
                + 4 * U32 * (np.abs(dot) + np.abs(bias) + M) + U_EXP2
            theta = np.where(live, theta, 0.0)
            tbar = (p * theta).sum(1, keepdims=True)
            Theta = theta.max(1, keepdims=True)
            e1 = np.exp(2 * Theta) * _dev_sum(np.ascontiguousarray(p * (theta + tbar)), np.ascontiguousarray(vv), np.ascontiguousarray(o))
            pv = p @ np.abs(vv)
            ao = np.abs(o)
            e2 = u_p * (pv + ao)
            e3 = 2 * a_p * (live.astype(np.float64) @ np.abs(vv) + n_i * ao) / l + a_op
            e4 = (n_i + 2 * -(-Nk // 32) + 3) * U32 * (pv + ao)
            out[b, h] = (1 + u_out) * (e1 + e2 + e3 + e4) + u_out * ao
    return out.transpose(0, 2, 1, 3).reshape(B, Nq, C)


def check(got, ref, bound):
    """(worst err / bound, index of the worst element); a non-finite output is infinitely wrong"""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return float("inf"), tuple(int(t) for t in np.argwhere(~np.isfinite(got))[0])
    r = np.abs(got - ref) / bound
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[i]), tuple(int(t) for t in i)


# ------------------------------------------------------------------------------------------------ inputs
FAMILIES = ("normal", "flat", "negative", "peaked", "peaked_last", "staircase", "large")


def peaked_positions(Nk):
    """first tile; the last key of a full tile; the first key of the next; the very last key (of a ragged last tile)"""
    return sorted({min(5, Nk - 1), min(TK - 1, Nk - 1), min(TK, Nk - 1), Nk - 1})


def staircase_levels(Nk):
    """the shared logit level of every key tile in exp2 units: up by 7 (below LAZY_THR), then by 9 (above), then 2 down and level"""
    return np.array([0.0, 7.0, 16.0] + [14.0] * 64)[:-(-Nk // TK)]


def make_inputs(family, seed, B, Nq, Nk, heads, dh, mode, scale=None):
    """q [B, Nq, C], k, v [B, Nk, C] fp32 of one family (issue text in the test modules), rounded to the compute type of `mode`.
    Every head gets the same construction on its own slice, so the families hold for every (sample, head)."""
    g = np.random.default_rng(seed)
    C = heads * dh
    scale = dh ** -0.5 if not scale else float(scale)
    n = lambda *shape: g.standard_normal(shape)
    q, k, v = n(B, Nq, C), n(B, Nk, C), n(B, Nk, C)
    if family == "flat":
        q *= 0.25; k *= 0.25; v += 4.0
    elif family == "negative":
        base = n(B, 1, C)
        q = base + 0.3 * q; k = -base + 0.3 * k; v += 1.0
    elif family in ("peaked", "peaked_last"):
        pos = peaked_positions(Nk) if family == "peaked" else [Nk - 1]
        for j, kp in enumerate(pos):       # key kp is 1.5 x the query it belongs to; under a causal mask that query must see it
            i = (j * Nq) // len(pos)
            i = min(Nq - 1, max(kp, i) if Nq == Nk else i)
            k[:, kp] = 1.5 * q[:, i]
    elif family == "staircase":
        # all queries share the component a * e per head (e a unit vector); the keys of tile t have c_t * e, so their logits sit at
        # scale * a * c_t = level_t / log2(e); what remains is noise of a few tenths of an exp2 unit (2.5 sigma of a tile's 64 keys)
        a = 4.0
        e = np.sign(n(1, 1, heads, dh)) / np.sqrt(dh)
        lev = np.repeat(staircase_levels(Nk), TK)[:Nk] / (LOG2E * scale * a)
        q = (a * e + 0.05 * q.reshape(B, Nq, heads, dh)).reshape(B, Nq, C)
        k = (lev[None, :, None, None] * e + 0.05 * k.reshape(B, Nk, heads, dh)).reshape(B, Nk, C)
    elif family == "large":
        q *= 4.0; k *= 4.0
    else:
        assert family == "normal", family
    return tuple(round_like(t.astype(np.float32), mode) for t in (q, k, v))


def staircase_rises(s):
    """from the reference's logits s [B, heads, Nq, Nk] (natural units): the rise of the row maximum from tile 0 to tile 1 and from
    tile 1 to tile 2, in exp2 units, as (min, max) pairs over all rows"""
    tm = np.stack([s[..., t:t + TK].max(-1) for t in range(0, s.shape[-1], TK)], -1) * LOG2E
    run = np.maximum.accumulate(tm, -1)
    r1, r2 = run[..., 1] - run[..., 0], run[..., 2] - run[..., 1]
    return (float(r1.min()), float(r1.max())), (float(r2.min()), float(r2.max()))


def make_relbias(seed, heads, Nk):
    """Toeplitz bias rows [heads, 2 Nk - 1], natural-log units: N(0, 2^2) plus a slope of its own per head"""
    g = np.random.default_rng(seed)
    d = np.arange(2 * Nk - 1) - (Nk - 1)
    slope = (np.arange(heads) + 1.0) * 0.05 * np.where(np.arange(heads) % 2, -1.0, 1.0)
    return (2.0 * g.standard_normal((heads, 2 * Nk - 1)) + slope[:, None] * d[None, :]).astype(np.float32)
