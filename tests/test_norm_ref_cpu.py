"""The bounds of tests/norm_ref.py have teeth, and sound implementations meet them (CPU only, NumPy / torch): for every
|mean| / std ratio and special input that test_norm_gpu.py feeds the HIP kernels, an independent fp32 two-pass GroupNorm /
LayerNorm and an emulation of each LayerNorm -> Linear path pass; the uncentred fp32-runs-of-16 statistics the fp32-input GroupNorm
kernels used to have, an unbiased variance and a dropped pixel fail."""
import numpy as np
import pytest

from tests import norm_ref as R

RATIOS = [0, 4, 16, 64, 256]
GN_SHAPES = [(2, 64, 16, 16), (2, 128, 5, 3)]   # 512 elements per group; 60 elements per group (odd pixel count)


def _gn_case(shape, kind, storage, eps, seed=3):
    x = R.gn_input(seed, shape, kind, storage)
    ga, be = R.affine(seed + 1, shape[1])
    ref = R.group_norm_ref(x, ga, be, eps)
    return x, ga, be, ref


@pytest.mark.parametrize("shape", GN_SHAPES)
@pytest.mark.parametrize("storage,kind", [(s, k) for s in ("f32", "f16", "bf16") for k in RATIOS + ["outlier"]
                                          if s == "f32" or k not in (64, 256)])   # 2-byte storage: asserted up to a ratio of 16
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_fp32_two_pass_groupnorm_meets_the_bound(shape, storage, kind, eps):
    x, ga, be, ref = _gn_case(shape, kind, storage, eps)
    E = R.gn_anchor(x, ga, be, eps, ref)
    worst, at = R.check(R.gn_two_pass_f32(x, ga, be, eps), ref, R.norm_bound(ref, E, 0.0))
    assert worst <= 1.0, (worst, at, E)
    # and rounded to a 2-byte output it meets that format's bound
    for out in ("f16", "bf16"):
        worst, at = R.check(R.round_to(R.gn_two_pass_f32(x, ga, be, eps), out), ref, R.norm_bound(ref, E, R.U_OUT[out]))
        assert worst <= 1.0, (out, worst, at, E)


@pytest.mark.parametrize("shape", GN_SHAPES)
@pytest.mark.parametrize("kind", RATIOS + ["outlier"])
def test_fp64_sums_repair_the_kernel_scheme(shape, kind):
    """sums and squares in fp64 from the first element, the rest of the kernels' arithmetic unchanged: inside the fp32 bound"""
    x, ga, be, ref = _gn_case(shape, kind, "f32", 1e-5)
    E = R.gn_anchor(x, ga, be, 1e-5, ref)
    worst, at = R.check(R.gn_runs_of_16_f32(x, ga, be, 1e-5, fp64_from_start=True), ref, R.norm_bound(ref, E, 0.0))
    assert worst <= 1.0, (worst, at, E)


FP16_RATIOS = [0, 1, 2, 2.5, 3, 3.5, 4, 5, 5.5, 6, 8, 12, 16]


@pytest.mark.parametrize("shape", [(2, 64, 16, 16), (1, 256, 32, 32), (2, 128, 8, 8)])   # whole runs of 16 pixels
@pytest.mark.parametrize("kind", FP16_RATIOS)
def test_pivoted_squares_repair_the_fp16_runs(shape, kind):
    """fp16 input, the bound of the coefficient form (u_out = 0), three seeds per case.  Plain fp32 runs of 16 squares of 22 bits each
    leave it from a ratio of about 2.5 up (1.4 x at 3 and 4, 2-5 x at 6 and 8).  With gn_run_flush's rule -- a run whose sum of squares
    exceeds 8 x its sum of squared deviations hands over the squares of x - pivot instead -- the emulation is inside at every ratio
    from 0 to 16, and a centred input still returns the very bits of the plain runs.  (The single-outlier input is not part of this
    sweep: its anchor E moves 5 x from seed to seed, and the rule leaves such a run, whose deviations are its outlier, plain.)"""
    some_plain_fail = False
    for seed in (3, 5, 7):
        x, ga, be, ref = _gn_case(shape, kind, "f16", 1e-5, seed)
        E = R.gn_anchor(x, ga, be, 1e-5, ref)
        bound = R.norm_bound(ref, E, 0.0)
        plain = R.gn_runs_of_16_f32(x, ga, be, 1e-5)
        piv = R.gn_runs_of_16_f32(x, ga, be, 1e-5, pivot=True)
        r_piv, at = R.check(piv, ref, bound)
        assert r_piv <= 1.0, (seed, r_piv, at, E)
        assert R.check(R.round_to(piv, "f16"), ref, R.norm_bound(ref, E, 2.0 ** -11))[0] <= 1.0
        some_plain_fail |= R.check(plain, ref, bound)[0] > 1.0
        if kind == 0:
            np.testing.assert_array_equal(piv, plain)
    if kind in (6, 8, 12, 16) and shape[2] * shape[3] >= 256:
        assert some_plain_fail


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("storage,u_out", [("f32", 0.0), ("f16", 2.0 ** -11), ("bf16", 2.0 ** -8)])
def test_constant_groups_meet_their_bound(storage, u_out, eps):
    shape = GN_SHAPES[0]
    x, ga, be, ref = _gn_case(shape, "const", storage, eps)
    assert np.abs(ref - be[None, :, None, None]).max() < 1e-9   # the reference of a constant group is beta
    bound = R.const_group_bound(x, ga, be, eps, u_out)
    # the kernels' scheme (fp64 sums for fp32 input, fp32 runs of 16 for 2-byte input): the fp64 mean of n equal values is exact, so
    # what is left is the rounding the bound names.  (A mean summed in fp32 is several ulps off on 512 equal values and does not
    # meet this bound: the independent fp32 two-pass is not held to it.)
    got = R.gn_runs_of_16_f32(x, ga, be, eps, fp64_from_start=storage == "f32")
    worst, at = R.check(R.round_to(got, storage), ref, bound)
    assert worst <= 1.0, (worst, at)
    # teeth: a mean that is off by 2^-20 |c| (16 fp32 ulps) is caught
    off = ref + 2.0 ** -20 * np.abs(x.astype(np.float64)) * np.abs(ga)[None, :, None, None] / np.sqrt(eps)
    assert R.check(off, ref, R.const_group_bound(x, ga, be, eps, 0.0))[0] > 1.0


def test_uncentred_fp32_runs_fail_the_fp32_bound_at_ratio_64():
    x, ga, be, ref = _gn_case(GN_SHAPES[0], 64, "f32", 1e-5)
    E = R.gn_anchor(x, ga, be, 1e-5, ref)
    worst, _ = R.check(R.gn_runs_of_16_f32(x, ga, be, 1e-5), ref, R.norm_bound(ref, E, 0.0))
    assert worst > 1.0, worst
    # while at a ratio of 0 the same scheme passes: the bound does not reject it for being a different summation order
    x, ga, be, ref = _gn_case(GN_SHAPES[0], 0, "f32", 1e-5)
    E = R.gn_anchor(x, ga, be, 1e-5, ref)
    assert R.check(R.gn_runs_of_16_f32(x, ga, be, 1e-5), ref, R.norm_bound(ref, E, 0.0))[0] <= 1.0


@pytest.mark.parametrize("u_out", [0.0, 2.0 ** -11, 2.0 ** -8])
def test_unbiased_variance_on_a_60_element_group_fails(u_out):
    x, ga, be, ref = _gn_case(GN_SHAPES[1], 0, "f32", 1e-5)
    E = R.gn_anchor(x, ga, be, 1e-5, ref)
    assert R.check(R.gn_two_pass_f32(x, ga, be, 1e-5, unbiased=True), ref, R.norm_bound(ref, E, u_out))[0] > 1.0


@pytest.mark.parametrize("shape", GN_SHAPES)
@pytest.mark.parametrize("u_out", [0.0, 2.0 ** -11, 2.0 ** -8])
def test_dropping_the_last_pixel_fails(shape, u_out):
    x, ga, be, ref = _gn_case(shape, 0, "f32", 1e-5)
    E = R.gn_anchor(x, ga, be, 1e-5, ref)
    assert R.check(R.gn_two_pass_f32(x, ga, be, 1e-5, drop_last=True), ref, R.norm_bound(ref, E, u_out))[0] > 1.0


@pytest.mark.parametrize("rows,C", [(9, 4), (5, 260), (100, 64), (6, 1536)])
@pytest.mark.parametrize("storage", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("ratio", RATIOS)
def test_fp32_two_pass_layernorm_meets_the_bound(rows, C, storage, ratio):
    x = R.ln_input(5, rows, C, ratio, storage)
    ga, be = R.affine(6, C)
    ref = R.layer_norm_ref(x, ga, be)
    E = R.ln_anchor(x, ga, be)
    worst, at = R.check(R.ln_two_pass_f32(x, ga, be), ref, R.norm_bound(ref, E, 0.0))
    assert worst <= 1.0, (worst, at, E)


@pytest.mark.parametrize("mode", list(R.MODES))
@pytest.mark.parametrize("folded,ratio", [(False, 0), (False, 4), (False, 16), (False, 64), (True, 0), (True, 4), (True, 16)])   # as asserted on the GPU
@pytest.mark.parametrize("M,K,N", [(77, 320, 40), (50, 640, 164)])
def test_ln_linear_emulations_meet_the_bound(mode, folded, ratio, M, K, N):
    S, T = R.MODES[mode]
    g = np.random.default_rng(9)
    h = R.ln_input(7, M, K, ratio, S)
    ga, be = R.affine(8, K)
    w = R.round_to((g.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32), T)
    bias = (0.1 * g.standard_normal(N)).astype(np.float32)
    ref = R.ln_linear_ref(h, ga, be, w, bias)
    E = R.ln_anchor(h)
    bound = R.ln_linear_bound(mode, folded, h, ga, be, w, bias, E)
    worst, at = R.check(R.ln_linear_emul(mode, folded, h, ga, be, w, bias), ref, bound)
    assert worst <= 1.0, (worst, at)
    # teeth: a path that forgot gamma, or beta, is outside even the widest of these bounds (the fold over an fp32 stream converted to
    # fp16 at a ratio of 16, whose uncentred operand rounding allows ~0.1 on outputs of order 1)
    assert R.check(R.ln_linear_emul(mode, folded, h, np.ones_like(ga), be, w, bias), ref, bound)[0] > 1.0
    assert R.check(R.ln_linear_emul(mode, folded, h, ga, np.zeros_like(be), w, bias), ref, bound)[0] > 1.0
