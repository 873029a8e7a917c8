"""The normalisation kernels against fp64, per element, on inputs whose groups / rows sit far from zero (tests/norm_ref.py holds the
references, the inputs and the bounds; tests/test_norm_ref_cpu.py shows that those bounds have teeth).

GroupNorm32: every implementation (two-pass gn_stats + gn_apply, the LDS-slab gn_fused_kernel, the register-resident gn_reg_kernel
in each of its NL / VB forms), each by nature and forced by the options gn_single / gn_reg, in all five engines (f32, f16x2, f16,
bf16, f16 with an fp32 residual stream), plus the split-K slab input form and the coefficient form.  Every case asserts stat
"gn_kernel": a shape that moves to another kernel fails instead of passing on the wrong code.  LayerNorm: every instantiation of
layernorm_kernel.  LayerNorm -> Linear: the kernel pair, the fold behind row_stats_kernel and the fold behind a producer GEMM's
stats_out epilogue (igemm tiles and the ring kernel), on ragged M and N.

Each test prints its worst err / bound ("[norm] ..." lines, pytest -s)."""
import numpy as np
import pytest

from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import weights as W
from tests import norm_ref as R
from tests.test_kernels_gpu import NORM_TOL

pytestmark = pytest.mark.gpu

TWO_PASS, LDS_SLAB, REGISTER = 1, 2, 3     # PD_GN_* of include/pdengine.h
KNAME = {TWO_PASS: "two-pass", LDS_SLAB: "lds-slab", REGISTER: "register"}
REG_SHAPES = [(2, 256, 8, 8), (1, 640, 4, 16), (1, 2560, 8, 8), (1, 1280, 16, 16), (2, 1920, 16, 16), (1, 256, 32, 32), (1, 640, 32, 32)]
SLAB_SHAPES = [(3, 320, 16, 16), (1, 960, 4, 4), (2, 128, 5, 3), (2, 192, 7, 9), (1, 64, 32, 32), (1, 320, 35, 36)]
TWO_PASS_SHAPES = [(1, 320, 36, 36), (1, 320, 64, 64), (1, 448, 6, 6), (2, 32, 8, 8)]
FORCED_TWO_PASS_SHAPES = [(2, 2560, 3, 5), (2, 320, 10, 10)]


@pytest.fixture(scope="module", params=list(R.MODES))
def eng(request):
    mode = request.param
    e = E.Engine(W.TINY, precision="f16" if mode == "f16s32" else mode, stream_f32=mode == "f16s32")
    e.mode = mode
    e.S, e.T = R.MODES[mode]
    yield e
    e.close()


def gn_kinds(storage):
    """ratios 0 .. 256 where the GroupNorm input is fp32, 0 .. 16 where it is 2-byte; one outlier, one constant-group input"""
    return ([0, 4, 16, 64, 256] if storage == "f32" else [0, 4, 16]) + ["outlier", "const"]


def expected_kernel(mode, shape, gn_single=True, gn_reg=True):
    """norm.hip's dispatch rule (gn_reg_vb, gn_slab_bundle, pd_engine::groupnorm), restated"""
    S, T = R.MODES[mode]
    B, C, H, Wd = shape
    HW, cpg = H * Wd, C // 32
    if not gn_single:
        return TWO_PASS
    if gn_reg and S == T and S != "f32" and HW in (64, 256, 1024):
        gb = cpg * 2
        for vb in (16, 8):
            if gb % vb == 0 and gb // vb <= (8 if HW == 1024 else 16) and (C * 2) % vb == 0:
                return REGISTER
    vec, ex = (4, 4) if S == "f32" else (8, 2)
    bc = cpg
    while bc % vec:
        bc += cpg
    if C % bc or bc // cpg > 4 or 960 % (bc // vec) or HW * bc * ex + 15 * 4 * 2 * 8 > 100 * 1024:
        return TWO_PASS
    return LDS_SLAB


def gn_case(shape, kind, storage, eps):
    x = R.gn_input(sum(shape) + 7 * (["outlier", "const"].index(kind) + 1 if isinstance(kind, str) else int(kind) + 3), shape, kind, storage)
    ga, be = R.affine(shape[1], shape[1])
    ref = R.group_norm_ref(x, ga, be, eps)
    anchor = None if kind == "const" else R.gn_anchor(x, ga, be, eps, ref)
    return x, ga, be, ref, anchor


def gn_bound(case, kind, eps, u_out):
    x, ga, be, ref, anchor = case
    return R.const_group_bound(x, ga, be, eps, u_out) if kind == "const" else R.norm_bound(ref, anchor, u_out)


def run_groupnorm(eng, shape, variants):
    """variants: [(label, {option: value}, expected kernel)]; every input kind and both eps through each of them"""
    u_out = R.U_OUT[eng.T]
    worst, fails = {}, []
    for eps in (1e-5, 1e-6):
        for kind in gn_kinds(eng.S):
            case = gn_case(shape, kind, eng.S, eps)
            x, ga, be, ref, anchor = case
            bound = gn_bound(case, kind, eps, u_out)
            for label, opts, want in variants:
                before = {k: eng.option(k) for k in opts}
                try:
                    for k, v in opts.items():
                        eng.set_option(k, v)
                    got = eng.op_groupnorm(x, ga, be, eps, False)
                    ran = eng.stat("gn_kernel")
                    got_silu = eng.op_groupnorm(x, ga, be, eps, True) if kind == 0 else None
                finally:
                    for k, v in before.items():
                        eng.set_option(k, v)
                assert ran == want, f"{shape} {label}: ran {KNAME.get(ran, ran)}, this case is about {KNAME[want]}"
                r, at = R.check(got, ref, bound)
                worst[label] = max(worst.get(label, 0.0), r)
                if not r <= 1.0:
                    fails.append((label, kind, eps, r, at, anchor))
                if got_silu is not None:   # SiLU variants: ratio 0, the suite's NORM_TOL per element (silu_f's __expf is not the subject)
                    sref = R.silu(ref)
                    tol = NORM_TOL["f16" if eng.mode == "f16s32" else eng.mode]
                    rs, at = R.check(got_silu, sref, tol * np.maximum(np.abs(sref), 1.0))
                    if not rs <= 1.0:
                        fails.append((label + "+silu", kind, eps, rs, at, anchor))
    for label, r in worst.items():
        print(f"[norm] groupnorm {eng.mode} {shape} {label}: worst err / bound {r:.3f}")
    assert not fails, f"{eng.mode} {shape}: (variant, input, eps, err / bound, at, E) {fails}"


@pytest.mark.parametrize("shape", REG_SHAPES)
def test_groupnorm_register_shapes(eng, shape):
    """gn_reg_kernel's NL 1 / 4 / 16, VB 16 / 8, nv 1 / 5 / 10 / 15 in the 2-byte modes (the fp32-storage modes take the LDS slab for
    these shapes), then the same shapes on the LDS slab (gn_reg 0) and on the two-pass kernels (gn_single 0): one bound for all three."""
    if eng.S == eng.T and eng.S != "f32":
        assert expected_kernel(eng.mode, shape) == REGISTER
    run_groupnorm(eng, shape, [("default", {}, expected_kernel(eng.mode, shape)),
                               ("gn_reg=0", {"gn_reg": 0}, LDS_SLAB),
                               ("gn_single=0", {"gn_single": 0}, TWO_PASS)])


@pytest.mark.parametrize("shape", SLAB_SHAPES)
def test_groupnorm_lds_slab_shapes(eng, shape):
    """gn_fused_kernel: fewer pixels than thread rows (2,192,7,9), odd pixel counts, the largest slab under the 100 KB budget"""
    run_groupnorm(eng, shape, [("default", {}, LDS_SLAB)])


@pytest.mark.parametrize("shape", TWO_PASS_SHAPES)
def test_groupnorm_two_pass_shapes(eng, shape):
    """gn_stats + gn_apply by nature: the first slab over the LDS budget, the 64 x 64 level, 7 vectors per pixel (no divisor of 960
    threads), one channel per group (two-pass in the 2-byte modes; its four-channel fp32 vector is still a legal slab bundle)."""
    want = expected_kernel(eng.mode, shape)
    assert want == TWO_PASS or (shape == (2, 32, 8, 8) and eng.S == "f32" and want == LDS_SLAB)
    run_groupnorm(eng, shape, [("default", {}, want)])


@pytest.mark.parametrize("shape", FORCED_TWO_PASS_SHAPES)
def test_groupnorm_two_pass_forced(eng, shape):
    """more channel vectors than threads; 12 chunks with a ragged last one"""
    run_groupnorm(eng, shape, [("gn_single=0", {"gn_single": 0}, TWO_PASS)])


@pytest.mark.parametrize("shape", [(1, 1280, 16, 16), (3, 320, 16, 16)])   # the register kernel (2-byte modes) and the LDS slab
@pytest.mark.parametrize("nslab", [1, 2, 4])
def test_groupnorm_from_split_k_slabs(eng, shape, nslab):
    """The SLAB input form in isolation: x = round_S(slab_0 + slab_1 + ... + bias + row) in fp32, in that order, rebuilt here; the
    result against fp64 and bit-identical to the stored-tensor form on that x."""
    B, C, H, Wd = shape
    g = np.random.default_rng(100 + nslab)
    ga, be = R.affine(C, C)
    want = expected_kernel(eng.mode, shape)
    assert want == (REGISTER if (shape[1] == 1280 and eng.S == eng.T != "f32") else LDS_SLAB)
    for with_extra in (False, True):
        # the parts sum to a ratio-4 input: groups N(0, s^2) shifted by +- 4 s, split over the slabs (and the bias / the row)
        target = R.gn_input(7, shape, 4, "f32").transpose(0, 2, 3, 1)
        bias = g.standard_normal(C).astype(np.float32) if with_extra else None
        row = (2 * g.standard_normal((B, C))).astype(np.float32) if with_extra else None
        slabs = (g.standard_normal((nslab, B, H, Wd, C)) * 3).astype(np.float32)
        rest = target.astype(np.float64) - slabs[:-1].astype(np.float64).sum(0)
        if with_extra:
            rest -= bias.astype(np.float64)[None, None, None, :] + row.astype(np.float64)[:, None, None, :]
        slabs[-1] = rest.astype(np.float32)
        acc = slabs[0].copy()
        for k in range(1, nslab):
            acc = (acc + slabs[k]).astype(np.float32)
        if with_extra:
            acc = (acc + bias[None, None, None, :]).astype(np.float32)
            acc = (acc + row[:, None, None, :]).astype(np.float32)
        x = R.round_to(np.ascontiguousarray(acc.transpose(0, 3, 1, 2)), eng.S)
        for eps in (1e-5, 1e-6):
            ref = R.group_norm_ref(x, ga, be, eps)
            bound = R.norm_bound(ref, R.gn_anchor(x, ga, be, eps, ref), R.U_OUT[eng.T])
            got = eng.op_groupnorm_slabs(slabs, ga, be, bias, row, eps)
            assert eng.stat("gn_kernel") == want
            r, at = R.check(got, ref, bound)
            print(f"[norm] groupnorm-slabs {eng.mode} {shape} nslab {nslab} extra {with_extra} eps {eps:g} {KNAME[want]}: err / bound {r:.3f}")
            assert r <= 1.0, (r, at)
            stored = eng.op_groupnorm(x, ga, be, eps, False)
            assert eng.stat("gn_kernel") == want
            np.testing.assert_array_equal(got, stored)
            np.testing.assert_array_equal(eng.op_groupnorm_slabs(slabs, ga, be, bias, row, eps, silu=True), eng.op_groupnorm(x, ga, be, eps, True))


def test_groupnorm_slabs_refused_without_a_single_kernel(eng):
    B, C, H, Wd = 1, 320, 36, 36   # the first slab over the LDS budget
    with pytest.raises(E.PdError, match="no single-kernel GroupNorm"):
        eng.op_groupnorm_slabs(np.zeros((1, B, H, Wd, C), np.float32), np.ones(C, np.float32), np.zeros(C, np.float32))


@pytest.mark.parametrize("shape", TWO_PASS_SHAPES + FORCED_TWO_PASS_SHAPES)
def test_groupnorm_coefficients(eng, shape):
    """gn_stats + gn_coef_kernel (what the GroupNorm-fused patch conv and st_front_kernel apply while staging): x a + b in fp64 against
    the GroupNorm bound with u_out = 0."""
    worst, fails = 0.0, []
    for eps in (1e-5, 1e-6):
        for kind in gn_kinds(eng.S):
            case = gn_case(shape, kind, eng.S, eps)
            x, ga, be, ref, anchor = case
            coef = eng.op_groupnorm_coef(x, ga, be, eps).astype(np.float64)
            got = x.astype(np.float64) * coef[:, :, 0][:, :, None, None] + coef[:, :, 1][:, :, None, None]
            r, at = R.check(got, ref, gn_bound(case, kind, eps, 0.0))
            worst = max(worst, r)
            if not r <= 1.0:
                fails.append((kind, eps, r, at, anchor))
    print(f"[norm] groupnorm-coef {eng.mode} {shape}: worst err / bound {worst:.3f}")
    assert not fails, f"{eng.mode} {shape}: (input, eps, err / bound, at, E) {fails}"


@pytest.mark.parametrize("rows,C", [(9, 4), (5, 260), (100, 64), (257, 640), (6, 1536), (3, 2048)])
def test_layernorm_kernel(eng, rows, C):
    """layernorm_kernel<.., 2 / 5 / 8> (C <= 512, <= 1280, <= 2048), rows that do not fill the last block, a vector count that does
    not fill a wave: a centred two-pass in fp32, held to 3 E (its output is fp32) at every ratio in every mode."""
    ga, be = R.affine(C + 1, C)
    worst, fails = 0.0, []
    for ratio in (0, 4, 16, 64, 256):
        x = R.ln_input(rows + C, rows, C, ratio, eng.S)
        ref = R.layer_norm_ref(x, ga, be)
        anchor = R.ln_anchor(x, ga, be)
        r, at = R.check(eng.op_layernorm(x, ga, be), ref, R.norm_bound(ref, anchor, 0.0))
        worst = max(worst, r)
        if not r <= 1.0:
            fails.append((ratio, r, at, anchor))
    print(f"[norm] layernorm {eng.mode} ({rows}, {C}): worst err / bound {worst:.3f}")
    assert not fails, f"{eng.mode}: (ratio, err / bound, at, E) {fails}"


# M, K, N: every K with every ragged M (the producer's stats_out rows and partials), every N of the set three times
LNL_SHAPES = [(77, 320, 40), (300, 320, 164), (1029, 320, 960), (77, 640, 164), (300, 640, 960), (1029, 640, 40),
              (77, 1280, 960), (300, 1280, 40), (1029, 1280, 164)]


def lnl_case(M, K, N, ratio, S, T):
    g = np.random.default_rng(M + K + N + int(ratio))
    ga, be = R.affine(K + 2, K)
    w = R.round_to((g.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32), T)
    bias = (0.1 * g.standard_normal(N)).astype(np.float32)
    h = R.ln_input(M + K, M, K, ratio, S)
    # the producer of mode 2: h = x w1^T + b1 (+ residual); the residual carries the row offsets (attn1.to_out), ratio 0 has none (proj_in)
    x = R.round_to(g.standard_normal((M, K)).astype(np.float32), T)
    w1 = R.round_to((g.standard_normal((K, K)) / np.sqrt(K)).astype(np.float32), T)
    b1 = (0.1 * g.standard_normal(K)).astype(np.float32)
    res = None if ratio == 0 else R.ln_input(M + K + 1, M, K, ratio, S)
    v = x.astype(np.float64) @ w1.astype(np.float64).T + b1.astype(np.float64)
    if res is not None:
        v = v + res.astype(np.float64)
    xw = np.abs(x).astype(np.float64) @ np.abs(w1).astype(np.float64).T   # for the producer's accumulation bound
    return ga, be, w, bias, h, x, w1, b1, res, v, xw


def check_row_stats(stats, vals, slack):
    """{sum, sum of squares} of every row as the fold received them, against fp64 of `vals`: fp32 accumulation of K values in any order
    plus the fold of up to 16 partials, plus `slack`, the distance of the summed values themselves from `vals`.  A partial written to
    another row's or another wave's slot is off by a whole tile's share of the row, orders of magnitude outside."""
    K = vals.shape[1]
    a = np.abs(vals)
    bs = (K + 16) * R.U32 * a.sum(1) + slack.sum(1)
    bq = (K + 16) * R.U32 * (a * a).sum(1) + (2 * a * slack + slack * slack).sum(1)
    rs, at = R.check(stats[:, 0], vals.sum(1), bs)
    assert rs <= 1.0, ("row sums", rs, at)
    rq, at = R.check(stats[:, 1], (vals * vals).sum(1), bq)
    assert rq <= 1.0, ("row sums of squares", rq, at)


def lnl_run(eng, mode, case):
    """one pd_op_ln_linear call -> (err / bound, where, statistics partials per row)"""
    ga, be, w, bias, h, x, w1, b1, res, v, xw = case
    if mode < 2:
        y, h_used, parts, stats = eng.op_ln_linear(mode, ga, be, w, bias, h=h)
        np.testing.assert_array_equal(h_used, h)   # the stream holds the rows as given
        producer = None
        assert parts == mode
        if mode == 1:
            check_row_stats(stats, h.astype(np.float64), np.zeros(h.shape))
    else:
        y, h_used, parts, stats = eng.op_ln_linear(2, ga, be, w, bias, x=x, w1=w1, b1=b1, residual=res)
        # the producer itself: h against fp64 (K 2^-24 accumulation on sum |x w1| and the rounding to S)
        hv = (x.shape[1] + 2) * R.U32 * (xw + np.abs(b1) + (0 if res is None else np.abs(res))) + (2.0 ** -20 if eng.mode == "f16x2" else 0.0) * xw
        hb = hv + R.U_FMT[eng.S] * (np.abs(v) + hv)
        rh, at = R.check(h_used, v, hb)
        assert rh <= 1.0, ("producer", rh, at)
        # the statistics the fold received: of the producer's fp32 value (its own epilogue), or of the stored h (row_stats_kernel
        # behind a split-K producer, one partial)
        if parts > 1:
            check_row_stats(stats, v, hv)
        else:
            check_row_stats(stats, h_used.astype(np.float64), np.zeros(h_used.shape))
        mean_v, rstd_v = R.layer_norm_stats(v)
        producer = np.abs(R.ln_linear_with_stats(h_used, mean_v, rstd_v, ga, be, w, bias) - R.ln_linear_ref(h_used, ga, be, w, bias))
    ref = R.ln_linear_ref(h_used, ga, be, w, bias)
    bound = R.ln_linear_bound(eng.mode, mode > 0, h_used, ga, be, w, bias, R.ln_anchor(h_used), producer)
    return R.check(y, ref, bound) + (parts,)


@pytest.mark.parametrize("M,K,N", LNL_SHAPES)
@pytest.mark.parametrize("ratio", [0, 4, 16, 64])
def test_layernorm_linear(eng, M, K, N, ratio):
    """LayerNorm -> Linear in isolation, three ways (pd_op_ln_linear), each against the bound derived next to norm_ref.ln_linear_bound.
    Ratios 0 / 4 / 16 are asserted.  At 64 the kernel pair is still asserted and the fold is printed only: its fp32 E[x^2] - mean^2
    statistics are past an fp16 ulp there (rstd off by ~8e-4 in emulation).

    The producer legs run with split-K off (splitk_max 1: K = 1280 is 20 K steps and would otherwise split on few tiles), so that
    which kernel ran is determined: both GEMMs on the ring kernel with ring 1000, neither with ring 0, and the statistics are the
    producing tile's own partials (more than one per row), checked directly against fp64.  K = 1280 runs once more on the engine's
    own plan, whatever it is (split-K slabs, the fold in the finalize pass, row_stats_kernel)."""
    case = lnl_case(M, K, N, ratio, eng.S, eng.T)
    two_byte = eng.S == eng.T and eng.S != "f32"
    runs = [("pair", 0, None, {}), ("fold/row_stats", 1, None, {})]
    runs += [("fold/producer ring", 2, 1000, {"splitk_max": 1}), ("fold/producer igemm", 2, 0, {"splitk_max": 1})] if two_byte else [("fold/producer", 2, None, {"splitk_max": 1})]
    if K >= 1024:
        runs.append(("fold/producer own plan", 2, None, {}))
    fails = []
    for label, mode, ring, opts in runs:
        try:
            if ring is not None:
                eng.set_option("ring", ring)
            for k, val in opts.items():
                eng.set_option(k, val)
            n0 = eng.stat("ring_launches")
            r, at, parts = lnl_run(eng, mode, case)
            moved = eng.stat("ring_launches") - n0
        finally:
            eng.set_option("ring", 80)
            eng.set_option("splitk_max", 16)
        if ring == 0:
            assert moved == 0, (label, moved)
        elif ring == 1000:
            assert moved == 2, (label, moved)    # producer and consumer
        if opts:
            assert parts > 1, (label, "the producer's epilogue left no statistics of its own", parts)
        print(f"[norm] ln-linear {eng.mode} M {M} K {K} N {N} ratio {ratio} {label}: err / bound {r:.3f} (ring launches {moved}, partials {parts})")
        if not r <= 1.0 and (mode == 0 or ratio <= 16):
            fails.append((label, r, at))
    assert not fails, f"{eng.mode}: (path, err / bound, at) {fails}"
