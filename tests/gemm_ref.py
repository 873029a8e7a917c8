"""fp64 reference, input families, case lists and a per-element error bound for the epilogue and addressing forms of the contraction
kernels (gemm.hip, gemm_ring.hip, the patch convs, the split-K finalize pass; pd_mma.h epilogue4_value / epilogue4_store).  Pure NumPy /
torch on the CPU, no engine import: shared by test_gemm_ref_cpu.py (which shows that the bound has teeth: every mistake of MUTANTS
exceeds it) and test_gemm_epilogue_gpu.py (which holds the HIP kernels to it through pd_op_linear_ex / pd_op_conv2d_ex).

The operation, on operands as stored (x, w in the compute type T, bias / rowvec / gate fp32, residual in its own type), for row
m = (sample s, token t) and column n:
    z    = sum_k x[arow(m)][k] w[n][k] + bias[n] + rowvec[s][n]
    v    = act(z) * scale * gate[s][n] + residual[m][n]
    C[crow(m)][n] = round_out(v)  for n < vt_begin,      VT[s][n - vt_begin][vt_tok_off + t] = round_out(v)  for n >= vt_begin
    arow(m) = s * a_sample_rows + a_row_off + t,  crow(m) = s * c_sample_rows + c_row_off + t   (the identity without a remap)
act 7 (gated tanh-GELU, packed [x | gate] weights): v = (x . w_x + b_x) * gelu_tanh(x . w_g + b_g), saturated to +-65504 on an fp16 store;
act 2 (GEGLU) the same with the erf GELU and no saturation.

Unit roundoffs (u = 2^-p, round to nearest even) and the accuracy taken for the special-function instructions:
    U32   = 2^-24   fp32: the MFMA accumulators and every operation of the epilogue
    u_T   : bf16 2^-8, f16 2^-11 (norm_ref.U_OUT); the output rounding of a 2-byte store; an fp16 store of a subnormal keeps 2^-25 absolute
    U_EXP = 2^-23   v_exp_f32 at one fp32 ulp of its result, as attn_ref takes it (no figure for it is at hand: a bound, not a measurement);
                    __expf(a) = v_exp_f32(a * log2 e) rounds its argument once more: relative error U_EXP + 2 |a| U32
    U_RCP = 2^-23   v_rcp_f32 at one ulp, as pd_mma.h states where it uses it
    ERF   = 1.5e-7 + 12 U32   gelu_fast's erf: the 1.5e-7 of Abramowitz-Stegun 7.1.26 that pd_common.h states, plus its fp32 evaluation: four
                    Horner steps on partial sums <= 1.5 (6 U32) and the reciprocal, the products and the exponential on e <= 1 (6 U32);
                    test_gemm_ref_cpu.py measures the same fp32 formula against fp64 over [-13, 13] and finds it inside
    TINY  = 2^-126  fp32 underflow, charged as TINY (1 + |z|): a quotient below the normal range may be flushed (2^-126), and once exp
                    overflows (t > 2^128) the quotient is -0 where the value is below |z| 2^-128

The error model, with P = x . w (fp64), S = sum_k |x_k| |w_k|, K the reduction length:
    e_acc = (n + 2 + splitk) U32 S      fp32 accumulation of n products in any order -- the worst case (n - 1) u sum |terms|, the MFMA's inner
                                        order is not ours to assume -- one rounding of each product in the fp32 mode, and one more
                                        addition per split-K slab.  n = K; f16x2: n = 4 K (four partial products per element) on
                                        S (1 + 2^-9), the magnitude of the hi / lo partial products
          + 2^-19 S                     f16x2 only, from pd_mma.h: an fp32 operand becomes hi = x truncated to fp16 (|x - hi| < 2^-10 |x|) and
                                        lo = RNE_fp16(x - hi), |x - hi - lo| <= 2^-21 |x|: 2 * 2^-21 S for the two operands; mma_x2 drops lo * lo,
                                        <= 2^-10 |x| 2^-10 |w| = 2^-20 of a product
          + 2^-25 (sum_k |x_k| + sum_k |w_k|)
                                        f16x2 only: a lo half below fp16's normal range (|x| < 2^-4) keeps half the smallest subnormal
    e_z   = e_acc + U32 (|P + bias| + |z|)                            + bias, + rowvec: one rounding each
    e_a   = L_act e_z + r_act(z) |act(z)| + a_act(z)                  L_act: the largest slope of the activation (1; SiLU and quick-GELU
                                        1.1; both GELUs 1.13), r_act / a_act its own relative / absolute evaluation error in fp32:
        (the relative error r_t of t = __expf(-a) reaches z / (1 + t) through t / (1 + t) = sig(-a))
        SiLU        z / (1 + __expf(-z)):            r = (U_EXP + 2 |z| U32) sig(-z) + 2 U32                 (1 + t, the division)
        quick-GELU  z / (1 + __expf(-1.702f z)):     r = (U_EXP + 4 * 1.702 |z| U32) sig(-1.702 z) + 2 U32   (the constant and the product round the argument)
        tanh-GELU   u = c fma(0.044715f z z, z, z), z / (1 + __expf(-2 u)):
                                                     r = (U_EXP + 16 |u| U32) sig(-2 u) + 2 U32, + U_RCP + U32 where the 2-byte branch multiplies by v_rcp_f32
                                                     (six roundings in u, each moving the exponential by 2 |u| U32, and __expf's own 2 |2u| U32)
        erf-GELU    gelu_fast:                       a = 0.5 |z| (ERF + 3 U32), r = 2 U32
        ReLU / none                                  nothing
      every one + TINY (1 + |z|).
    e_v   = |scale gate| e_a + 2 U32 |act(z) scale gate| + U32 |v|    * scale, * gate, + residual: one rounding each
    bound = (1 + u_out) e_v (1 + 2^-20) + u_out |v| (+ 2^-25 on an fp16 store)     (1 + 2^-20: the second-order terms of the above)
    gated: with e_x, e_g the e_z of the two halves and G = gelu_tanh(g): e_v = |G| e_x + |x| (1.13 e_g + r |G|) + U32 |x G|, clipped like the value.
Unit roundoffs and operation counts are the only constants: nothing here is fitted to what a kernel returns."""
import collections

import numpy as np
import torch

from tests.norm_ref import U32, U_OUT, round_to

STORAGE = {"f32": "f32", "f16x2": "f32", "f16": "f16", "bf16": "bf16"}      # the compute type T (= the stream type S in these four modes)
U_EXP = 2.0 ** -23
U_RCP = 2.0 ** -23
ERF = 1.5e-7 + 12 * U32
TINY = 2.0 ** -126
F16_MAX = 65504.0
ACT_NONE, ACT_SILU, ACT_GEGLU, ACT_QUICK, ACT_TANH, ACT_RELU, ACT_ERF, ACT_GATED = range(8)     # Activation of csrc/pd_common.h
L_ACT = {ACT_NONE: 1.0, ACT_SILU: 1.1, ACT_QUICK: 1.1, ACT_TANH: 1.13, ACT_RELU: 1.0, ACT_ERF: 1.13}
REMAP = 33            # rows of the other stream ahead of this call's in a joint buffer (c_row_off / a_row_off / vt_tok_off)
FAMILIES = ("normal", "per_sample", "cancel", "ragged_bias", "act_edges")

# One call of pd_op_linear_ex.  res_dt / out_dt: None / "f32" / "T" / "S"; c_remap / a_remap: sample_rows = tokens + REMAP, row_off = REMAP
Spec = collections.namedtuple("Spec", "family B tokens K N act bias rowvec gate scale res_dt out_dt vt_begin vt_extra vt_tok_off c_remap a_remap ldc_extra",
                              defaults=(ACT_NONE, True, False, False, 1.0, None, "f32", 0, 0, 0, False, False, 0))


def round_like(x, mode, dt="T"):
    """x as the engine of `mode` holds it in dt: "f32", or the compute / stream type"""
    x = np.asarray(x, np.float32)
    return x if dt == "f32" else round_to(x, STORAGE[mode])


def out_fmt(mode, dt):
    return "f32" if dt == "f32" else STORAGE[mode]


def trunc_to(x, fmt):
    """x (fp64) rounded toward zero to fmt -- the wrong rounding of the `truncate` mutant"""
    if fmt == "f32":
        return np.asarray(x, np.float64)
    r = round_to(np.asarray(x, np.float32), fmt).astype(np.float64)
    x = np.asarray(x, np.float64)
    over = np.abs(r) > np.abs(x)
    if fmt == "bf16":
        step = np.float32(r).view(np.uint32)
        down = ((step - np.uint32(0x10000)).view(np.float32)).astype(np.float64)
    else:
        h = r.astype(np.float16).view(np.uint16)
        down = (h - np.uint16(1)).view(np.float16).astype(np.float64)
    return np.where(over, down, r)


# ------------------------------------------------------------------------------------------------ activations (fp64)
def _erf(x):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x, np.float64))).numpy()


def gelu_tanh(z, cubic=True):
    u = 0.7978845608028654 * (z + (0.044715 * z ** 3 if cubic else 0.0))
    with np.errstate(over="ignore"):
        return z / (1.0 + np.exp(-2.0 * u))


def act_ref(z, act, mutant=None):
    with np.errstate(over="ignore"):
        if act == ACT_SILU:
            return z / (1.0 + np.exp(-z))
        if act == ACT_QUICK:
            return z / (1.0 + np.exp(-1.702 * z))
        if act == ACT_TANH:
            return gelu_tanh(z, mutant != "gelu_no_cubic")
        if act == ACT_ERF:
            return 0.5 * z * (1.0 + _erf(z * 0.7071067811865476))
        if act == ACT_RELU:
            return np.maximum(z, 0.0)
    assert act == ACT_NONE, act
    return z


def act_error(z, act, fast_div=False):
    """(relative, absolute) evaluation error of the activation at z, module docstring; the error of t = exp(-a) reaches z / (1 + t) through
    t / (1 + t) = 1 / (1 + exp(a))"""
    az = np.abs(z)
    with np.errstate(over="ignore"):
        if act == ACT_SILU:
            return (U_EXP + 2 * az * U32) / (1.0 + np.exp(z)) + 2 * U32, TINY * (1 + az)
        if act == ACT_QUICK:
            return (U_EXP + 4 * 1.702 * az * U32) / (1.0 + np.exp(1.702 * z)) + 2 * U32, TINY * (1 + az)
        if act == ACT_TANH:
            u = 0.7978845608028654 * (z + 0.044715 * z ** 3)
            return (U_EXP + 16 * np.abs(u) * U32) / (1.0 + np.exp(2.0 * u)) + 2 * U32 + ((U_RCP + U32) if fast_div else 0.0), TINY * (1 + az)
    if act == ACT_ERF:
        return 2 * U32, 0.5 * az * (ERF + 3 * U32) + TINY * (1 + az)
    return 0.0, 0.0


def gelu_fast_f32(x):
    """pd_common.h gelu_fast in NumPy fp32 (np.exp for __expf, a division for v_rcp_f32)"""
    f = np.float32
    x = np.asarray(x, f)
    z = np.abs(x) * f(0.70710678118654752)
    t = f(1.0) / (f(0.3275911) * z + f(1.0))
    poly = f(1.061405429) * t + f(-1.453152027)
    poly = poly * t + f(1.421413741)
    poly = poly * t + f(-0.284496736)
    poly = poly * t + f(0.254829592)
    e = poly * t * np.exp(-z * z)
    return f(0.5) * x * (f(1.0) + np.copysign(f(1.0) - e, x))


def act_f32(z, act):
    """the kernels' fp32 formulas in NumPy fp32 (gemm_emul)"""
    f = np.float32
    z = np.asarray(z, f)
    with np.errstate(over="ignore"):
        if act == ACT_SILU:
            return z / (f(1.0) + np.exp(-z))
        if act == ACT_QUICK:
            return z / (f(1.0) + np.exp(f(-1.702) * z))
        if act == ACT_TANH:
            u = f(0.7978845608028654) * (f(0.044715) * z * z * z + z)
            return z / (f(1.0) + np.exp(f(-2.0) * u))
        if act == ACT_ERF:
            return gelu_fast_f32(z)
        if act == ACT_RELU:
            return np.maximum(z, f(0.0))
    return z


# ------------------------------------------------------------------------------------------------ inputs
def make_inputs(spec, mode, seed=0):
    """x [M, K], w [N or 2N, K], bias, rowvec / gate [B, N], residual [M, N] of one family, each rounded to the type the engine holds it in.
    normal: N(0, 1) rows against N(0, 1 / K) weights.  per_sample: every sample's rowvec and gate rows have an offset and a slope of their
    own of several units.  cancel: residual = -scale gate act(z), so the output is what the rounding of the residual leaves.
    ragged_bias: a sawtooth of period 16 and step 0.25 over n, so a column group shifted by 4 is 1.0 (or 3.0) off.  act_edges: the
    pre-activations spread over [-12, 12] through the bias (gated: the gate half; row 1 scaled so that its products leave the fp16 range)."""
    s = spec
    g = np.random.default_rng(1000 * FAMILIES.index(s.family) + 131 * s.B + 17 * s.tokens + 7 * s.K + 3 * s.N + 11 * s.act + seed)
    M, packed = s.B * s.tokens, s.act in (ACT_GEGLU, ACT_GATED)
    Nw = 2 * s.N if packed else s.N
    x = g.standard_normal((M, s.K))
    w = g.standard_normal((Nw, s.K)) / np.sqrt(s.K)
    bias = 0.1 * g.standard_normal(Nw)
    n = np.arange(s.N)
    smp = np.arange(s.B)[:, None]
    rowvec = g.standard_normal((s.B, s.N))
    gate = 1.0 + 0.5 * g.standard_normal((s.B, s.N))
    if s.family == "per_sample":
        rowvec = 4.0 * (smp + 1) * np.where(smp % 2, -1.0, 1.0) + 3.0 * (smp + 1) * n[None, :] / s.N + 0.1 * rowvec
        gate = 2.0 + 1.5 * smp + (smp + 1.0) * n[None, :] / s.N
    elif s.family == "ragged_bias":
        bias = 0.25 * (np.arange(Nw) % 16) - 2.0 + 0.01 * bias
    elif s.family == "act_edges":
        w = 0.3 * w
        bias = g.permutation(np.linspace(-12.0, 12.0, s.N))
        if packed:
            bias = np.concatenate([0.1 * g.standard_normal(s.N), bias])
            x[1] *= 1.0e4
    x, w = round_like(x, mode), round_like(w, mode)
    inp = dict(x=x, w=w, bias=bias.astype(np.float32) if s.bias else None, rowvec=rowvec.astype(np.float32) if s.rowvec else None,
               gate=gate.astype(np.float32) if s.gate else None, residual=None)
    if s.res_dt:
        if s.family == "cancel":
            r = -values(inp, s._replace(res_dt=None), mode)
        else:
            r = g.standard_normal((M, s.N))
        inp["residual"] = round_like(r, mode, s.res_dt)
    for a in inp.values():
        if a is not None:
            a.setflags(write=False)
    return inp


# ------------------------------------------------------------------------------------------------ reference (fp64)
MUTANTS = ("gate_next_sample", "rowvec_next_sample", "gate_after_residual", "scale_after_residual", "c_row_off_dropped", "a_row_off_dropped",
           "vt_tok_off_dropped", "vt_token_off1", "vt_first_group_skipped", "bias_n_plus_4", "residual_ldc", "last_row_next_sample", "gelu_no_cubic",
           "truncate")


def _geometry(s):
    M = s.B * s.tokens
    ldc = s.N + s.ldc_extra
    c_rows = s.tokens + REMAP if s.c_remap else 0
    a_rows = s.tokens + REMAP if s.a_remap else 0
    vt_ld = -(-(s.vt_tok_off + s.tokens) // 8) * 8 + s.vt_extra
    return M, ldc, c_rows, a_rows, vt_ld


def values(inp, spec, mode, mutant=None):
    """v [M, N] in fp64, before the output rounding, as epilogue4_value states it (mutant: one of the value-side mistakes)"""
    s = spec
    M, ldc, c_rows, a_rows, _ = _geometry(s)
    f8 = lambda a: None if a is None else np.asarray(a, np.float64)
    x, w, bias, rowvec, gate, res = (f8(inp[k]) for k in ("x", "w", "bias", "rowvec", "gate", "residual"))
    m = np.arange(M)
    smp, tok = m // s.tokens, m % s.tokens
    if a_rows:     # the joint buffer the kernel gathers from: other rows NaN
        joint = np.full((s.B * a_rows, s.K), np.nan)
        joint[smp * a_rows + REMAP + tok] = x
        x = joint[smp * a_rows + (0 if mutant == "a_row_off_dropped" else REMAP) + tok]
    if mutant == "last_row_next_sample":       # a tile that straddles two samples takes the sample of its next row
        smp = np.minimum((m + 1) // s.tokens, s.B - 1)
    z = x @ w.T
    if bias is not None:
        z = z + (np.roll(bias, -4) if mutant == "bias_n_plus_4" else bias)
    if s.act in (ACT_GEGLU, ACT_GATED):
        xh, gh = z[:, :s.N], z[:, s.N:]
        if s.act == ACT_GEGLU:
            return xh * (0.5 * gh * (1.0 + _erf(gh * 0.7071067811865476)))
        v = xh * gelu_tanh(gh)
        return np.clip(v, -F16_MAX, F16_MAX) if out_fmt(mode, s.out_dt) == "f16" else v
    if rowvec is not None:
        z = z + rowvec[(smp + 1) % s.B if mutant == "rowvec_next_sample" else smp]
    a = act_ref(z, s.act, mutant)
    gt = 1.0 if gate is None else gate[(smp + 1) % s.B if mutant == "gate_next_sample" else smp]
    if res is not None and mutant == "residual_ldc":      # row stride of C where the residual's own was meant
        flat = res.reshape(-1)
        res = flat[(m[:, None] * ldc + np.arange(s.N)[None, :]) % flat.size]
    r = 0.0 if res is None else res
    if mutant == "gate_after_residual":
        return (a * s.scale + r) * gt
    if mutant == "scale_after_residual":
        return (a * gt + r) * s.scale
    return a * s.scale * gt + r


def place(v, spec, mutant=None):
    """What pd_op_linear_ex hands back for stored values v [M, N]: the C and V^T buffers start as NaN, the kernel writes v where
    epilogue4_store puts it (mutant: one of the addressing mistakes), the hook reads the call's own rows / columns / tokens.
    Returns (y [M, ncol], vt [B, N - vt_begin, tokens] or None)."""
    s = spec
    M, ldc, c_rows, a_rows, vt_ld = _geometry(s)
    m = np.arange(M)
    smp, tok = m // s.tokens, m % s.tokens
    ncol = s.vt_begin or s.N
    own = smp * c_rows + REMAP + tok if c_rows else m
    crow = smp * c_rows + tok if (c_rows and mutant == "c_row_off_dropped") else own
    C = np.full((s.B * c_rows if c_rows else M, ldc), np.nan)
    vt_from = s.vt_begin + (4 if mutant == "vt_first_group_skipped" else 0)
    C[crow, :ncol] = v[:, :ncol]
    if not s.vt_begin:
        return C[own, :ncol], None
    if vt_from > s.vt_begin:
        C[crow, s.vt_begin:vt_from] = v[:, s.vt_begin:vt_from]
    VT = np.full((s.B, s.N - s.vt_begin, vt_ld + 1), np.nan)
    t_at = (0 if mutant == "vt_tok_off_dropped" else s.vt_tok_off) + tok + (1 if mutant == "vt_token_off1" else 0)
    cols = np.arange(vt_from, s.N)
    VT[smp[:, None], (cols - s.vt_begin)[None, :], t_at[:, None]] = v[:, vt_from:]
    return C[own, :ncol], VT[:, :, s.vt_tok_off:s.vt_tok_off + s.tokens]


def gemm_ref(inp, spec, mode, mutant=None):
    """(y, vt) of the call in fp64; mutant: one of MUTANTS, the mistakes a kernel could make"""
    assert mutant is None or mutant in MUTANTS
    v = values(inp, spec, mode, mutant)
    if mutant == "truncate":
        v = trunc_to(v, out_fmt(mode, spec.out_dt))
    return place(v, spec, mutant)


# ------------------------------------------------------------------------------------------------ bound
def accumulate_error(mode, S, K, ax, aw, splitk=1):
    """e_acc of the module docstring.  S = |x| . |w|; ax [M, 1] / aw [1, N] = sum_k |x_k| / sum_k |w_k|"""
    if mode == "f16x2":
        return (4 * K + 2 + splitk) * U32 * S * (1 + 2.0 ** -9) + 2.0 ** -19 * S + 2.0 ** -25 * (ax + aw)
    return (K + 2 + splitk) * U32 * S


def epilogue_bound(mode, P, e_acc, bias, rowvec_rows, gate_rows, residual, act, scale, out, fast_div=None):
    """bound [.., N] for v = act(P + bias + rowvec) scale gate + residual stored as `out` ("f32" / "f16" / "bf16"); every array
    broadcasts against P"""
    b = 0.0 if bias is None else bias
    rv = 0.0 if rowvec_rows is None else rowvec_rows
    z = P + b + rv
    e_z = e_acc + U32 * (np.abs(P + b) + np.abs(z))
    a = act_ref(z, act)
    rel, ab = act_error(z, act, (out != "f32") if fast_div is None else fast_div)
    e_a = L_ACT[act] * e_z + rel * np.abs(a) + ab
    sg = scale * (1.0 if gate_rows is None else gate_rows)
    v = a * sg + (0.0 if residual is None else residual)
    e_v = np.abs(sg) * e_a + 2 * U32 * np.abs(a * sg) + U32 * np.abs(v)
    return _store_bound(e_v, v, out)


def _store_bound(e_v, v, out):
    u = U_OUT[out]
    return (1 + u) * e_v * (1 + 2.0 ** -20) + u * np.abs(v) + (2.0 ** -25 if out == "f16" else 0.0)


def gemm_bound(inp, spec, mode, splitk=1):
    """The per-element bound of the module docstring, shaped like gemm_ref's (y, vt)."""
    s = spec
    f8 = lambda a: None if a is None else np.asarray(a, np.float64)
    x, w, bias, rowvec, gate, res = (f8(inp[k]) for k in ("x", "w", "bias", "rowvec", "gate", "residual"))
    smp = np.arange(s.B * s.tokens) // s.tokens
    out = out_fmt(mode, s.out_dt)
    P, S = x @ w.T, np.abs(x) @ np.abs(w).T
    e_acc = accumulate_error(mode, S, s.K, np.abs(x).sum(1)[:, None], np.abs(w).sum(1)[None, :], splitk)
    if s.act in (ACT_GEGLU, ACT_GATED):
        z = P + (0.0 if bias is None else bias)
        e_z = e_acc + U32 * np.abs(z)
        (xh, gh), (e_x, e_g) = (z[:, :s.N], z[:, s.N:]), (e_z[:, :s.N], e_z[:, s.N:])
        if s.act == ACT_GATED:
            G = gelu_tanh(gh)
            rel, ab = act_error(gh, ACT_TANH, False)
        else:
            G = 0.5 * gh * (1.0 + _erf(gh * 0.7071067811865476))
            rel, ab = act_error(gh, ACT_ERF)
        e_v = np.abs(G) * e_x + (np.abs(xh) + e_x) * (1.13 * e_g + rel * np.abs(G) + ab) + U32 * np.abs(xh * G)
        bd = _store_bound(e_v, np.clip(xh * G, -F16_MAX, F16_MAX) if (s.act == ACT_GATED and out == "f16") else xh * G, out)
    else:
        bd = epilogue_bound(mode, P, e_acc, bias, None if rowvec is None else rowvec[smp], None if gate is None else gate[smp], res, s.act, s.scale, out)
    return place(bd, s._replace(c_remap=False, ldc_extra=0, vt_tok_off=0, vt_extra=0))


def gemm_emul(inp, spec, mode):
    """An independent evaluation in the kernels' own arithmetic -- NumPy fp32 products and sums (f16x2: hi + lo operands), the epilogue
    one fp32 operation at a time, the stated fp32 formula of each activation, the output rounded to its type -- shaped like gemm_ref's."""
    s = spec
    f = np.float32
    x, w = inp["x"], inp["w"]
    if mode == "f16x2":
        def split(t):
            hi = t.astype(np.float16).astype(f)
            return hi + (t - hi).astype(np.float16).astype(f)
        x, w = split(x), split(w)
    smp = np.arange(s.B * s.tokens) // s.tokens
    z = (x.astype(f) @ w.astype(f).T).astype(f)
    if inp["bias"] is not None:
        z = z + inp["bias"]
    out = out_fmt(mode, s.out_dt)
    if s.act in (ACT_GEGLU, ACT_GATED):
        xh, gh = z[:, :s.N], z[:, s.N:]
        v = xh * (act_f32(gh, ACT_TANH) if s.act == ACT_GATED else gelu_fast_f32(gh))
        if s.act == ACT_GATED and out == "f16":
            v = np.clip(v, -F16_MAX, F16_MAX)
    else:
        if inp["rowvec"] is not None:
            z = z + inp["rowvec"][smp]
        v = act_f32(z, s.act) * f(s.scale)
        if inp["gate"] is not None:
            v = v * inp["gate"][smp]
        if inp["residual"] is not None:
            v = v + inp["residual"]
    assert v.dtype == f
    return place(round_to(v, out).astype(np.float64), s._replace(c_remap=False, ldc_extra=0, vt_tok_off=0, vt_extra=0))


def check(got, ref, bound):
    """(worst err / bound, index of the worst element) over the parts of a (y, vt) pair; a non-finite output is infinitely wrong"""
    worst = (0.0, ())
    for part, (g_, r_, b_) in enumerate(zip(got, ref, bound)):
        if r_ is None:
            continue
        g_ = np.asarray(g_, np.float64)
        if g_.shape != r_.shape or not np.isfinite(g_).all():
            bad = np.argwhere(~np.isfinite(g_))[0] if g_.shape == r_.shape else ()
            return float("inf"), (part,) + tuple(int(t) for t in bad)
        r = np.abs(g_ - r_) / b_
        i = np.unravel_index(int(np.argmax(r)), r.shape)
        if float(r[i]) > worst[0]:
            worst = (float(r[i]), (part,) + tuple(int(t) for t in i))
    return worst


# ------------------------------------------------------------------------------------------------ convolutions
def conv_products(x, w, stride=1):
    """(P, S, sum |x|, sum |w|, K) of conv2d(x, w, padding k // 2) in fp64, NCHW; operands as stored"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))
    k = w.shape[-1]
    conv = lambda a, b: torch.nn.functional.conv2d(t(a), t(b), None, stride, k // 2).numpy()
    ax = conv(np.abs(x), np.ones((1,) + w.shape[1:]))
    aw = np.abs(np.asarray(w, np.float64)).sum((1, 2, 3))[None, :, None, None]
    return conv(x, w), conv(np.abs(x), np.abs(w)), ax, aw, w.shape[1] * k * k


def conv_ref_bound(mode, products, bias, rowvec, residual, act, scale, out, splitk=1):
    """(fp64 reference, bound) of act(conv + bias + rowvec[b]) scale + residual from conv_products' arrays"""
    P, S, ax, aw, K = products
    e_acc = accumulate_error(mode, S, K, ax, aw, splitk)
    col = lambda a: None if a is None else np.asarray(a, np.float64)[None, :, None, None]
    rv = None if rowvec is None else np.asarray(rowvec, np.float64)[:, :, None, None]
    res = None if residual is None else np.asarray(residual, np.float64)
    z = P + (0.0 if bias is None else col(bias)) + (0.0 if rv is None else rv)
    ref = act_ref(z, act) * scale + (0.0 if res is None else res)
    return ref, epilogue_bound(mode, P, e_acc, col(bias), rv, None, res, act, scale, out)


# ------------------------------------------------------------------------------------------------ the GPU case lists
# One GPU run: a Spec and how it is dispatched.  tile / splitk: options gemm_tile / gemm_splitk; ring: None (option ring 0: igemm) or
# (ring_tile, ring_pp) with option ring 1000
Case = collections.namedtuple("Case", "spec tile splitk ring", defaults=(0, 1, None))
TILES = {"f32": (0, 1), "f16x2": (0, 1), "f16": (0, 1, 2, 3, 4), "bf16": (0, 1, 2, 3, 4)}
TILE_ROWS = {0: 128, 1: 256, 2: 128, 3: 256, 4: 256}


def tile_cases(tile):
    """The epilogue and addressing forms on one tile.  M = 3 x 77 where the tile has 128 rows and 3 x 100 where it has 256, so a tile
    straddles two samples; N from {164, 320, 384} (tile 4, 256 x 192: 384); K from {72, 200, 320}, and 1280 unsplit and in 4 slices
    (split launches take the 128- and 256-row tiles 0 / 1)."""
    tok = 77 if TILE_ROWS[tile] == 128 else 100
    n = (lambda i: 384) if tile == 4 else (lambda i: (164, 320, 384)[i % 3])
    k = lambda i: (72, 200, 320)[i % 3]
    S = lambda fam, i, **kw: Spec(fam, 3, tok, k(i + tile), n(i), **kw)
    c = [Case(S("per_sample", 0, rowvec=True), tile),                                                             # bias + rowvec
         Case(S("ragged_bias", 1, scale=0.75, res_dt="f32", out_dt="T", ldc_extra=28), tile),                    # scale + residual, each res_dt
         Case(S("cancel", 2, scale=0.75, res_dt="T"), tile),
         Case(S("normal", 3, scale=1.5, res_dt="S", out_dt="T"), tile),
         Case(S("per_sample", 4, gate=True, res_dt="S", out_dt="T"), tile),                                      # MM: gate + residual
         Case(S("per_sample", 5, gate=True, res_dt="f32", c_remap=True, a_remap=True, ldc_extra=28), tile),       # ... with the row remaps
         Case(S("cancel", 6, gate=True, scale=0.5, res_dt="T", out_dt="T", c_remap=True, a_remap=True), tile),
         Case(S("per_sample", 7, rowvec=True, gate=True, out_dt="T", a_remap=True, ldc_extra=28), tile),
         Case(Spec("per_sample", 3, tok, 1280, n(1), rowvec=True, scale=0.75, res_dt="S", out_dt="T"), tile, 1),
         Case(Spec("per_sample", 3, tok, 1280, n(0), rowvec=True, gate=True, res_dt="f32", c_remap=True, a_remap=True), tile, 1)]
    if tile == 3:     # the 256 x 320 tile is not built with the MM extras (the launcher runs 256 x 160 there: tile 1's cases): plain forms only
        c = [x for x in c if not (x.spec.gate or x.spec.c_remap or x.spec.a_remap)]
    if tile < 2:
        c += [Case(Spec("per_sample", 3, tok, 1280, n(1), rowvec=True, scale=0.75, res_dt="S", out_dt="T", ldc_extra=28), tile, 4),
              Case(Spec("cancel", 3, tok, 1280, n(2), gate=True, res_dt="T", c_remap=True, a_remap=True), tile, 4),
              Case(Spec("ragged_bias", 3, tok, 1280, n(0), scale=0.75, res_dt="f32", out_dt="T"), tile, 2)]
    return c


def vt_cases(tile):
    """The V^T side output on one tile: vt_begin = 2N/3 (N 384) and N/2 (N 320; on the 256 x 192 tile N 384 again), 77 and 64 tokens, pad
    tokens, the other stream's tokens ahead (with the row remap that goes with them: the MM instantiations, which the 256 x 320 tile
    does not have), fp32 and 2-byte."""
    tok = (77, 64)
    c = []
    for i, (N, vb) in enumerate(((384, 256), (384, 192) if tile == 4 else (320, 160))):
        for j, out in enumerate(("f32", "T")):
            c.append(Case(Spec("normal", 3, tok[(i + j) % 2], (72, 200, 320)[(i + j) % 3], N, out_dt=out, vt_begin=vb, vt_extra=8 * ((i + j) % 2)), tile))
            if tile != 3:
                c.append(Case(Spec("ragged_bias", 3, tok[(i + j + 1) % 2], (200, 320, 72)[(i + j) % 3], N, out_dt=out, vt_begin=vb,
                                   vt_extra=8 * ((i + j + 1) % 2), vt_tok_off=REMAP, c_remap=True), tile))
    return c


def act_cases(mode):
    """Every activation on the instantiation that owns it, pre-activations over [-12, 12]"""
    two = STORAGE[mode] != "f32"
    S = lambda act, N=320, tok=77, **kw: Spec("act_edges", 3, tok, 200, N, act, **kw)
    c = [Case(S(ACT_SILU), 0), Case(S(ACT_SILU, out_dt="T"), 2 if two else 1), Case(S(ACT_QUICK), 0), Case(S(ACT_QUICK, N=164, out_dt="T"), 1),
         Case(S(ACT_TANH), 0), Case(S(ACT_TANH, out_dt="T"), 0), Case(S(ACT_TANH, N=384, tok=100, out_dt="T"), 4 if two else 1), Case(S(ACT_TANH, N=164, tok=100), 1),
         Case(S(ACT_ERF), 0), Case(S(ACT_ERF, N=164, tok=100, out_dt="T"), 1),
         Case(S(ACT_RELU), 0), Case(S(ACT_RELU, N=164, tok=100, out_dt="T"), 1),
         Case(S(ACT_GATED), 0), Case(S(ACT_GATED, tok=100, out_dt="T"), 1)]
    return c


def ring_cases():
    """What ring_gemm_eligible admits of the above: 2-byte residual, V^T, 2-byte output, an output row stride, SiLU and quick-GELU.  ring =
    (option ring_tile, option ring_pp); the 128 x 160 tile takes its ping-pong form from 40 K steps on, so that pair runs K = 2560"""
    c = []
    for i, (rt, pp) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1), (4, 1))):
        tok = 100 if rt == 1 else 77
        K, N = (128, 320)[i % 2], (164, 320)[(i + 1) % 2]
        K, K2 = (2560, 2560) if (rt, pp) == (0, 1) else (K, (320, 128)[i % 2])
        c += [Case(Spec("cancel", 3, tok, K, N, scale=0.75, res_dt="T", out_dt="T", ldc_extra=28 * (i % 2)), 0, 1, (rt, pp)),
              Case(Spec("normal", 3, tok, K2, 320, out_dt="T", vt_begin=160, vt_extra=8), 0, 1, (rt, pp)),
              Case(Spec("act_edges", 3, tok, K, N, (ACT_SILU, ACT_QUICK)[i % 2], res_dt="S", out_dt="T", ldc_extra=28 * ((i + 1) % 2)), 0, 1, (rt, pp))]
    return c


def ring_launched(c):
    """launch_ring_gemm's tile for a ring case (plan_gemm): 2 / 3 are the ping-pong forms of 0 / 1, taken from 40 K steps of 64 on and
    for 256-row tiles that give every CU at most one"""
    rt, pp = c.ring
    return rt + 2 if pp and rt < 2 and (c.spec.K // 64 >= 40 or rt == 1) else rt


def all_cases(mode):
    c = []
    for t in TILES[mode]:
        c += tile_cases(t)
    for t in TILES[mode]:
        c += vt_cases(t)
    c += act_cases(mode)
    if STORAGE[mode] != "f32":
        c += ring_cases()
    return c


def shapes(mode):
    """the distinct (B, tokens, K, N) of the GPU case list"""
    return sorted({(c.spec.B, c.spec.tokens, c.spec.K, c.spec.N) for c in all_cases(mode)})
