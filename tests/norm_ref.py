"""fp64 references, inputs and per-element error bounds for the normalisation kernels (GroupNorm32, LayerNorm and
LayerNorm -> Linear).  Pure NumPy / torch on the CPU: shared by test_norm_ref_cpu.py (which shows that the bounds have teeth and
that sound implementations meet them) and test_norm_gpu.py (which holds the HIP kernels to them).

Engine modes and their number formats (S: the residual stream a norm reads, T: the compute type it writes / a GEMM contracts):
    f32     S fp32, T fp32            f16x2   S fp32, T fp32 (GEMM operands split into fp16 hi + lo pairs)
    f16     S fp16, T fp16            bf16    S bf16, T bf16            f16s32  S fp32, T fp16 (Engine(..., stream_f32=True))

The anchor of every statistics bound is E: the largest absolute error of torch's own fp32 F.group_norm / F.layer_norm against
fp64 on the same input, measured where it is used.  A kernel may be 3 E off (a different but sound summation order: an
independent fp32 two-pass and two repaired forms of the kernels' scheme sit at <= 1.0 E, the uncentred fp32-runs-of-16 scheme
at 4.2 E for |mean| / std = 16 and 23 E for 64) plus the rounding of its output format."""
import numpy as np
import torch

U32 = 2.0 ** -24
MODES = {"f32": ("f32", "f32"), "f16x2": ("f32", "f32"), "f16": ("f16", "f16"), "bf16": ("bf16", "bf16"), "f16s32": ("f32", "f16")}
U_OUT = {"f32": 0.0, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}    # rounding of a norm's output (an fp32 result is the anchor's own format)
U_FMT = {"f32": U32, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}    # unit roundoff of a format
GROUPS = 32


def round_to(x, fmt):
    """x (fp32) rounded to fmt and back: what the engine stores."""
    x = np.ascontiguousarray(x, np.float32)
    if fmt == "bf16":
        return torch.from_numpy(x).bfloat16().float().numpy()
    if fmt == "f16":
        return x.astype(np.float16).astype(np.float32)
    return x


# ------------------------------------------------------------------------------------------------ inputs
def gn_input(seed, shape, kind, storage):
    """[B, C, H, W] fp32, rounded to `storage`.  kind: a number r -- every (sample, group) is N(0, s^2), s in [0.5, 2], shifted by
    +- r s; "outlier" -- N(0, 1) with one element of one group at 1000 (fp32 storage) / 200 (2-byte storage); "const" -- every
    (sample, group) equal to its own constant, none of them representable (0.1 in the first)."""
    B, C, H, W = shape
    g = np.random.default_rng(seed)
    n = (C // GROUPS) * H * W
    x = g.standard_normal((B, GROUPS, n))
    if kind == "outlier":
        x[B - 1, GROUPS // 2, n // 3] = 1000.0 if storage == "f32" else 200.0
    elif kind == "const":
        c = g.uniform(-3.0, 3.0, (B, GROUPS, 1))
        c[0, 0, 0] = 0.1
        x = np.broadcast_to(c, x.shape).copy()
    else:
        s = g.uniform(0.5, 2.0, (B, GROUPS, 1))
        sign = np.where(g.random((B, GROUPS, 1)) < 0.5, -1.0, 1.0)
        x = x * s + sign * float(kind) * s
    x = x.reshape(B, GROUPS, C // GROUPS, H, W).reshape(B, C, H, W)
    return round_to(x.astype(np.float32), storage)


def ln_input(seed, rows, C, ratio, storage):
    """[rows, C] fp32, rounded to `storage`: every row N(0, s^2), s in [0.5, 2], shifted by +- ratio s."""
    g = np.random.default_rng(seed)
    s = g.uniform(0.5, 2.0, (rows, 1))
    sign = np.where(g.random((rows, 1)) < 0.5, -1.0, 1.0)
    return round_to((g.standard_normal((rows, C)) * s + sign * float(ratio) * s).astype(np.float32), storage)


def affine(seed, C):
    g = np.random.default_rng(seed)
    return (1 + 0.3 * g.standard_normal(C)).astype(np.float32), (0.3 * g.standard_normal(C)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ references (fp64)
def group_norm_ref(x, gamma, beta, eps, groups=GROUPS):
    """GroupNorm (biased variance over each sample's group) of x [B, C, H, W] in fp64."""
    B, C, H, W = x.shape
    v = x.astype(np.float64).reshape(B, groups, -1)
    mean = v.mean(-1, keepdims=True)
    var = ((v - mean) ** 2).mean(-1, keepdims=True)
    y = ((v - mean) / np.sqrt(var + float(eps))).reshape(B, C, H, W)
    return y * gamma.astype(np.float64)[None, :, None, None] + beta.astype(np.float64)[None, :, None, None]


def layer_norm_stats(x, eps=1e-5):
    v = x.astype(np.float64)
    mean = v.mean(-1, keepdims=True)
    var = ((v - mean) ** 2).mean(-1, keepdims=True)
    return mean, 1.0 / np.sqrt(var + float(eps))


def layer_norm_ref(x, gamma, beta, eps=1e-5):
    mean, rstd = layer_norm_stats(x, eps)
    return (x.astype(np.float64) - mean) * rstd * gamma.astype(np.float64) + beta.astype(np.float64)


def ln_linear_ref(h, gamma, beta, w, bias, eps=1e-5):
    y = layer_norm_ref(h, gamma, beta, eps) @ w.astype(np.float64).T
    return y if bias is None else y + bias.astype(np.float64)


def silu(x):
    return x / (1.0 + np.exp(-x))


# ------------------------------------------------------------------------------------------------ anchors
def gn_anchor(x, gamma, beta, eps, ref=None):
    """E: max |torch fp32 F.group_norm - fp64| on this input with these parameters."""
    ref = group_norm_ref(x, gamma, beta, eps) if ref is None else ref
    t = torch.nn.functional.group_norm(torch.from_numpy(np.ascontiguousarray(x, np.float32)), GROUPS, torch.from_numpy(gamma),
                                       torch.from_numpy(beta), float(eps)).numpy()
    return float(np.abs(t.astype(np.float64) - ref).max())


def ln_anchor(x, gamma=None, beta=None, eps=1e-5):
    """E: max |torch fp32 F.layer_norm - fp64| on this input; without gamma / beta, the error of the normalised value itself."""
    C = x.shape[-1]
    tg = None if gamma is None else torch.from_numpy(gamma)
    tb = None if beta is None else torch.from_numpy(beta)
    t = torch.nn.functional.layer_norm(torch.from_numpy(np.ascontiguousarray(x, np.float32)), (C,), tg, tb, float(eps)).numpy()
    one, zero = np.ones(C, np.float32), np.zeros(C, np.float32)
    ref = layer_norm_ref(x, one if gamma is None else gamma, zero if beta is None else beta, eps)
    return float(np.abs(t.astype(np.float64) - ref).max())


# ------------------------------------------------------------------------------------------------ bounds
def norm_bound(ref, E, u_out):
    """GroupNorm / LayerNorm output, per element: 3 E + u_out max(|ref|, 1)."""
    return 3.0 * E + u_out * np.maximum(np.abs(ref), 1.0)


def const_group_bound(x, gamma, beta, eps, u_out):
    """Every element of a group equals c: the reference is beta, and what a kernel may add is the rounding of the stored fp32 mean
    (2^-24 |c|, doubled for the coefficient form b = beta - mean a that rounds once more at that magnitude, and doubled again as
    margin) times the largest possible rstd, 1 / sqrt(eps), times |gamma|."""
    B, C, H, W = x.shape
    c = np.abs(x.astype(np.float64))
    g = np.abs(gamma.astype(np.float64))[None, :, None, None]
    b = np.abs(beta.astype(np.float64))[None, :, None, None]
    return 2.0 ** -22 * c * g / np.sqrt(float(eps)) + u_out * np.maximum(b, 1.0) + np.zeros((B, C, H, W))


def check(got, ref, bound):
    """(worst err / bound, index of the worst element); finite values only count"""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return float("inf"), None
    r = np.abs(got - ref) / bound
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[i]), i


# LayerNorm -> Linear, element (m, n).  Notation: h the stored input rows (exact in fp64), mu_m / r_m their fp64 mean / rstd,
# z = (h - mu) r the normalised value, L = z gamma + beta, y = sum_k L_mk w_nk + bias_n the reference.  w is what the engine holds
# (the test rounds it to T first), u_T the unit roundoff of the compute type, u = 2^-24 that of fp32.  Per engine mode, u_op is the
# relative error of bringing an fp32 value into the form the MFMA contracts: 0 in f32 (fp32 MACs), 2^-20 in f16x2 (hi truncated to
# 11 bits, lo to the next 11; the dropped lo * lo product and an fp16-subnormal lo are covered by the 2^-24 (sum|A| + sum|W|) term),
# u_T where a value is rounded to a 2-byte T.  E is the anchor of the normalised value: max |torch fp32 layer_norm(h) - z|.
#
# Unfused (mode 0): the GEMM contracts A = round_T(fp32 L) against w.
#   |A - L| <= 3 E |gamma| (statistics: what the LayerNorm bound allows) + 4 u (|z gamma| + |beta|) (the kernel's fp32 multiply, multiply,
#              add, and one to spare) + u_op |L|                                                       =: a_mk
#   |y_got - y| <= sum_k a_mk |w_nk| + u_op' sum_k |L_mk w_nk|    (u_op' = 2^-20 in f16x2, whose w is split as well; else 0)
#                + (K + 2) u (sum_k |L_mk w_nk| + |bias_n|)       (fp32 accumulation of K products, in any order, and the bias add)
#                + u_T (|y| + the above)                          (y is stored in T)
#
# Folded (modes 1, 2): the GEMM contracts the raw rows h (u_op applies only where S != T or the operand is split) against
# W' = round_T(fp32(w gamma)), and the epilogue forms r (acc - mu colsum_n) + bias'_n with colsum_n = sum_k W'_nk in fp32 and
# bias'_n = bias_n + sum_k beta_k w_nk in fp32.  colsum is that of the rounded W', so a rounding of W' meets (h - mu), not h:
#   W' rounding:       sum_k |z_mk| (u + u_T' + u_op') |w_nk gamma_k|      (u_T' = u_T for a 2-byte T, 0 for fp32)
#   A conversion:      r_m sum_k u_opA |h_mk| |w_nk gamma_k|               (u_opA = u_T in f16s32, 2^-20 in f16x2, else 0)
#   accumulation:      (K + 4) u r_m (sum_k |h_mk w_nk gamma_k| + |mu_m| sum_k |w_nk gamma_k|)
#                      -- the operand is r h, uncentred: this is the price of the fold and it grows with |mu| / sigma; the second sum is
#                      colsum's own fp32 accumulation, which the epilogue multiplies by mu r; + 4 for the epilogue's multiplies and adds
#                      + (K + 2) u (sum_k |beta_k w_nk| + |bias_n|) for bias'
#   statistics:        3 E sum_k |gamma_k w_nk|                            (an error d of the normalised value, the same for every k up to
#                      sign, reaches y through sum_k d gamma_k w_nk)
#   producer (mode 2): the statistics are those of the producer's fp32 value v, taken before v is rounded to S and stored as h, while the
#                      reference normalises h.  With v recomputed in fp64 that difference is known exactly:
#                      |y(h; mu_v, r_v) - y(h; mu_h, r_h)|, passed in as `producer`.
#   output:            u_T (|y| + the above)
def ln_linear_bound(mode, folded, h, gamma, beta, w, bias, E, producer=None, eps=1e-5):
    S, T = MODES[mode]
    K = h.shape[1]
    h = h.astype(np.float64); w = w.astype(np.float64)
    g = gamma.astype(np.float64); b = beta.astype(np.float64)
    ab = 0.0 if bias is None else np.abs(bias.astype(np.float64))[None, :]
    mu, r = layer_norm_stats(h, eps)
    z = (h - mu) * r
    y = ln_linear_ref(h, gamma, beta, w, bias, eps)
    x2 = mode == "f16x2"
    u_t2 = U_FMT[T] if T != "f32" else 0.0
    split = 2.0 ** -20 if x2 else 0.0
    aw = np.abs(w)
    if not folded:
        L = z * g + b
        a = 3.0 * E * np.abs(g) + 4 * U32 * (np.abs(z * g) + np.abs(b)) + (u_t2 + split) * np.abs(L)
        LW = np.abs(L) @ aw.T
        t = a @ aw.T + split * LW + (K + 2) * U32 * (LW + ab)
        if x2:
            t = t + U32 * (np.abs(L).sum(1, keepdims=True) + aw.sum(1)[None, :])
    else:
        wg = np.abs(w * g)
        u_opa = U_FMT[T] if (S == "f32" and T != "f32") else split
        hW = np.abs(h) @ wg.T
        swg = wg.sum(1)[None, :]
        t = np.abs(z) @ ((U32 + u_t2 + split) * wg).T + r * u_opa * hW
        t = t + (K + 4) * U32 * r * (hW + np.abs(mu) * swg) + (K + 2) * U32 * ((np.abs(b)[None, :] @ aw.T) + ab)
        t = t + 3.0 * E * swg
        if x2:
            t = t + U32 * (r * np.abs(h).sum(1, keepdims=True) + swg)
        if producer is not None:
            t = t + producer
    return t + U_FMT[T] * (np.abs(y) + t)


def ln_linear_with_stats(h, mean, rstd, gamma, beta, w, bias):
    """fp64 LayerNorm -> Linear of h with given row statistics (the `producer` term of ln_linear_bound)."""
    y = ((h.astype(np.float64) - mean) * rstd * gamma.astype(np.float64) + beta.astype(np.float64)) @ w.astype(np.float64).T
    return y if bias is None else y + bias.astype(np.float64)


# ------------------------------------------------------------------------------------------------ emulations (CPU test)
def gn_two_pass_f32(x, gamma, beta, eps, drop_last=False, unbiased=False):
    """An independent fp32 two-pass GroupNorm in NumPy; drop_last / unbiased are the deliberately wrong forms the bounds must catch."""
    B, C, H, W = x.shape
    v = x.astype(np.float32).reshape(B, GROUPS, C // GROUPS, H * W)
    s = v[..., :-1] if drop_last else v
    n = np.float32(s.shape[2] * s.shape[3])
    mean = (s.sum((2, 3), keepdims=True, dtype=np.float32) / n).astype(np.float32)
    d = (s - mean).astype(np.float32)
    var = ((d * d).sum((2, 3), keepdims=True, dtype=np.float32) / (n - np.float32(1) if unbiased else n)).astype(np.float32)
    rstd = (np.float32(1) / np.sqrt(var + np.float32(eps))).astype(np.float32)
    y = ((v - mean) * rstd).reshape(B, C, H, W)
    return (y * gamma[None, :, None, None] + beta[None, :, None, None]).astype(np.float32)


def gn_runs_of_16_f32(x, gamma, beta, eps, fp64_from_start=False, pivot=False, threshold=8.0):
    """The scheme of the GroupNorm kernels: var = E[x^2] - mean^2 from uncentred sums, fp32 runs of 16 values per channel folded in
    fp64, y = fma(x, a, b) with a = rstd gamma, b = beta - mean a in fp32.  fp64_from_start: sums and squares in fp64 from the first
    element (the fp32-input kernels).  pivot: the fp16-input kernels -- a run that sits off centre (its sum of squares above `threshold` x its
    sum of squared deviations) hands over the squares of x - pivot instead, put back in fp64 (norm.hip, gn_run_flush)."""
    B, C, H, W = x.shape
    HW = H * W
    v = x.astype(np.float32).reshape(B, C, HW)
    if fp64_from_start:
        d = v.astype(np.float64)
        s, q = d.sum(-1), (d * d).sum(-1)
    else:
        pad = (-HW) % 16
        vp = np.concatenate([v, np.zeros((B, C, pad), np.float32)], -1).reshape(B, C, -1, 16)
        rs = np.zeros(vp.shape[:3], np.float32); rq = np.zeros(vp.shape[:3], np.float32)
        for i in range(16):
            rs = (rs + vp[..., i]).astype(np.float32)
            rq = (vp[..., i] * vp[..., i] + rq).astype(np.float32)     # (fmaf rounds once; the product of two fp32 rounds here too)
        rq = rq.astype(np.float64)
        if pivot:
            assert pad == 0
            p = vp[..., 0]
            pq = np.zeros(vp.shape[:3], np.float32)
            for i in range(16):
                d = (vp[..., i] - p).astype(np.float32)
                pq = (d * d + pq).astype(np.float32)
            sd = (rs - np.float32(16) * p).astype(np.float32)
            dev = (pq - sd * sd / np.float32(16)).astype(np.float32)
            p64 = p.astype(np.float64)
            refined = pq.astype(np.float64) + p64 * (2.0 * (rs.astype(np.float64) - 16 * p64) + 16 * p64)
            rq = np.where(rq.astype(np.float32) > np.float32(threshold) * dev, refined, rq)
        s, q = rs.astype(np.float64).sum(-1), rq.sum(-1)
    cpg = C // GROUPS
    n = float(cpg * HW)
    S, Q = s.reshape(B, GROUPS, cpg).sum(-1), q.reshape(B, GROUPS, cpg).sum(-1)
    mean = S / n
    var = np.maximum(Q / n - mean * mean, 0.0)
    mean_f, rstd_f = mean.astype(np.float32), (1.0 / np.sqrt(var + float(eps))).astype(np.float32)
    a = (np.repeat(rstd_f, cpg, 1) * gamma[None, :]).astype(np.float32)
    b = (beta[None, :] - (np.repeat(mean_f, cpg, 1) * a).astype(np.float32)).astype(np.float32)
    y = (v.astype(np.float64) * a[..., None].astype(np.float64) + b[..., None].astype(np.float64)).astype(np.float32)   # one rounding: fma
    return y.reshape(B, C, H, W)


def ln_two_pass_f32(x, gamma, beta, eps=1e-5):
    v = x.astype(np.float32)
    C = np.float32(v.shape[1])
    mean = (v.sum(1, keepdims=True, dtype=np.float32) / C).astype(np.float32)
    d = (v - mean).astype(np.float32)
    rstd = (np.float32(1) / np.sqrt((d * d).sum(1, keepdims=True, dtype=np.float32) / C + np.float32(eps))).astype(np.float32)
    return (((d * rstd).astype(np.float32) * gamma).astype(np.float32) + beta).astype(np.float32)


def _contract(mode, a, w):
    """fp32-accumulated product of operands already in the form the mode contracts (f16x2: the hi + lo split keeps 22 bits)"""
    if mode == "f16x2":
        def split(t):
            hi = t.astype(np.float16).astype(np.float32)
            return hi + (t - hi).astype(np.float16).astype(np.float32)
        a, w = split(a), split(w)
    return (a.astype(np.float32) @ w.astype(np.float32).T).astype(np.float32)


def ln_linear_emul(mode, folded, h, gamma, beta, w, bias, eps=1e-5):
    """Each LayerNorm -> Linear path in its stated arithmetic (see ln_linear_bound); h already in S, w already in T."""
    S, T = MODES[mode]
    bias = np.zeros(w.shape[0], np.float32) if bias is None else bias
    if not folded:
        y = _contract(mode, round_to(ln_two_pass_f32(h, gamma, beta, eps), T), w) + bias
        return round_to(y.astype(np.float32), T)
    K = np.float32(h.shape[1])
    v = h.astype(np.float32)
    s = v.sum(1, keepdims=True, dtype=np.float32)
    q = (v * v).sum(1, keepdims=True, dtype=np.float32)
    mean = (s / K).astype(np.float32)
    var = np.maximum((q / K).astype(np.float32) - (mean * mean).astype(np.float32), np.float32(0))
    rstd = (np.float32(1) / np.sqrt(var + np.float32(eps))).astype(np.float32)
    wp = round_to((w * gamma[None, :]).astype(np.float32), T)
    colsum = wp.sum(1, dtype=np.float32)
    bias2 = (bias + (w * beta[None, :]).astype(np.float32).sum(1, dtype=np.float32)).astype(np.float32)
    acc = _contract(mode, round_to(v, T), wp)
    y = (rstd * (acc - (mean * colsum[None, :]).astype(np.float32)).astype(np.float32)).astype(np.float32) + bias2
    return round_to(y.astype(np.float32), T)
