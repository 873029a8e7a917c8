"""The epilogue and addressing forms of the contraction kernels against fp64, per element (tests/gemm_ref.py holds the reference, the input
families, the case lists and the bound; tests/test_gemm_ref_cpu.py shows that the bound has teeth and that the lists cover what they claim).

gemm.hip / gemm_ring.hip through pd_op_linear_ex in the forms the networks launch and pd_op_linear cannot express: the V^T side output
with pad tokens and a token offset, the per-sample row and gate, residuals in every type, 2-byte outputs, an output row stride, the
joint-buffer row remaps of C and A, every activation on the instantiation that owns it -- on every tile the mode has (options
"gemm_tile" / "gemm_splitk" put M = 231 / 300 on the 256-row tiles and on the split-K finalize pass).  The patch convs, igemm and the
finalize pass with the time-embedding row and ReLU through pd_op_conv2d_ex.  Every case asserts the stats "gemm_family", "gemm_tile" and
"gemm_splitk", so a case that drifts onto other code fails instead of passing there, and that no output element outside the call's own
changed (every buffer starts as NaN).

Each test prints its worst err / bound ("[gemm] ..." lines, pytest -s)."""
import functools

import numpy as np
import pytest

from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import weights as W
from tests import gemm_ref as R
from tests.test_kernels_gpu import PATCH1, PATCH2, PATCH4, PATCH_DEFAULTS, PATCH_SPLIT, PATCH_UNSPLIT

pytestmark = pytest.mark.gpu

RING, IGEMM = 4, 5                 # PD_GEMM_* of include/pdengine.h
GEMM_DEFAULTS = {"gemm_tile": -1, "gemm_splitk": -1, "ring": 80, "ring_tile": -1, "ring_pp": 1, "splitk_max": 16}


@pytest.fixture(scope="module", params=["f32", "f16x2", "f16", "bf16"])
def eng(request):
    e = E.Engine(W.TINY, precision=request.param)
    e.mode = request.param
    e.two_byte = request.param in ("f16", "bf16")
    yield e
    e.close()


@pytest.fixture(scope="module", params=["f16", "bf16"])
def eng2(request):
    e = E.Engine(W.TINY, precision=request.param)
    e.mode = request.param
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def inputs(storage, spec):
    """inputs and reference of a call, shared by the modes of one storage type and by every kernel it runs on; never modified"""
    inp = R.make_inputs(spec, storage)
    ref = R.gemm_ref(inp, spec, storage)
    return inp, ref


@functools.lru_cache(maxsize=None)
def bound_of(mode, spec, splitk):
    inp, _ = inputs(R.STORAGE[mode], spec)
    return R.gemm_bound(inp, spec, mode, splitk)


def call(eng, spec, inp):
    s = spec
    remap = s.tokens + R.REMAP
    return eng.op_linear_ex(inp["x"], inp["w"], inp["bias"], act=s.act, scale=s.scale, residual=inp["residual"], res_dt=s.res_dt or "f32",
                            out_dt=s.out_dt, rows_per_sample=s.tokens, rowvec=inp["rowvec"], gate=inp["gate"], vt_begin=s.vt_begin,
                            vt_extra=s.vt_extra, vt_tok_off=s.vt_tok_off, c_sample_rows=remap if s.c_remap else 0,
                            c_row_off=R.REMAP if s.c_remap else 0, a_sample_rows=remap if s.a_remap else 0,
                            a_row_off=R.REMAP if s.a_remap else 0, ldc_extra=s.ldc_extra)


def run_one(eng, c, ring=None):
    """One case under its options: ((y, vt), touched).  Asserts where it ran."""
    inp, _ = inputs(R.STORAGE[eng.mode], c.spec)
    opts = {"gemm_tile": c.tile, "gemm_splitk": c.splitk, "ring": 0} if ring is None else {"ring": 1000, "ring_tile": ring[0], "ring_pp": ring[1], "splitk_max": 1}      # (the ring kernel takes unsplit launches: K = 2560 at these M would split)
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        n0 = eng.stat("ring_launches")
        y, vt, touched = call(eng, c.spec, inp)
        ran = (eng.stat("gemm_family"), eng.stat("gemm_tile"), eng.stat("gemm_splitk"), eng.stat("ring_launches") - n0, eng.stat("gemm_ring_tile"))
    finally:
        for k, v in GEMM_DEFAULTS.items():
            eng.set_option(k, v)
    # (tile -1: the plan's own.  A ring launch: which of its five forms, ping-pong included, stat "gemm_ring_tile")
    want = (IGEMM, c.tile if c.tile >= 0 else ran[1], c.splitk, 0, -1) if ring is None else (RING, 0, 1, 1, R.ring_launched(c))
    assert ran == want, f"{c}: ran (family, tile, splitk, ring launches, ring tile) {ran}, this case is about {want}"
    return (y, vt), touched


def run_cases(eng, what, cases):
    """Every case where it says it runs; prints the worst err / bound per (kernel, tile), fails with every case past it."""
    worst, fails = {}, []
    for c in cases:
        _, ref = inputs(R.STORAGE[eng.mode], c.spec)
        bound = bound_of(eng.mode, c.spec, c.splitk)
        got, touched = run_one(eng, c, c.ring)
        key = f"ring tile {R.ring_launched(c)}" if c.ring else f"igemm tile {c.tile}" + (f" splitk {c.splitk}" if c.splitk > 1 else "")
        assert touched == 0, f"{c}: {touched} output elements outside the call's own rows / columns / tokens changed"
        if c.ring:      # the ring kernel sums in igemm_kernel's order and shares its epilogue: the same bits
            base, _ = run_one(eng, c._replace(tile=-1, splitk=1))
            assert all(b is None or np.array_equal(g, b) for g, b in zip(got, base)), f"{c}: the ring kernel and igemm_kernel differ"
        r, at = R.check(got, ref, bound)
        if r > worst.get(key, (0.0,))[0]:
            worst[key] = (r, c, at)
        if not r <= 1.0:
            fails.append((key, c, r, at))
    for key, (r, c, at) in sorted(worst.items()):
        print(f"[gemm] {what} {eng.mode} {key}: worst err / bound {r:.3f} at (part, ...) {at} of {c.spec}")
    assert not fails, f"{eng.mode} {what}: err / bound > 1 in {len(fails)} runs: " + "; ".join(f"{k} {c} {r:.3f} at {at}" for k, c, r, at in fails[:6])


def test_tiles(eng):
    for t in R.TILES[eng.mode]:
        run_cases(eng, "epilogue forms", R.tile_cases(t))


def test_vt_side_output(eng):
    for t in R.TILES[eng.mode]:
        run_cases(eng, "V^T", R.vt_cases(t))


def test_activations(eng):
    run_cases(eng, "activations", R.act_cases(eng.mode))


def test_ring(eng2):
    run_cases(eng2, "ring", R.ring_cases())
    # a per-sample row or gate is not the ring kernel's: the dispatch keeps such a call on igemm_kernel
    try:
        eng2.set_option("ring", 1000)
        for kw in (dict(rowvec=True), dict(gate=True)):
            spec = R.Spec("per_sample", 3, 77, 128, 320, **kw)
            inp, ref = inputs(R.STORAGE[eng2.mode], spec)
            n0 = eng2.stat("ring_launches")
            y, vt, touched = call(eng2, spec, inp)
            assert eng2.stat("ring_launches") == n0 and eng2.stat("gemm_family") == IGEMM and eng2.stat("gemm_ring_tile") == -1 and touched == 0
            assert R.check((y, vt), ref, bound_of(eng2.mode, spec, 1))[0] <= 1.0
    finally:
        eng2.set_option("ring", 80)


def test_plain_hooks_are_the_extended_ones_at_their_defaults(eng):
    g = np.random.default_rng(5)
    x = g.standard_normal((130, 200), dtype=np.float32)
    w = (g.standard_normal((164, 200), dtype=np.float32) / 14).astype(np.float32)
    b = g.standard_normal(164, dtype=np.float32) * 0.1
    y, vt, touched = eng.op_linear_ex(x, w, b)
    assert np.array_equal(eng.op_linear(x, w, b), y) and vt is None and touched == 0
    assert np.array_equal(eng.op_linear(x, w, b, a_silu=True), eng.op_linear_ex(x, w, b, a_silu=True)[0])
    w2 = (g.standard_normal((320, 200), dtype=np.float32) / 14).astype(np.float32)
    b2 = g.standard_normal(320, dtype=np.float32) * 0.1
    assert np.array_equal(eng.op_linear(x, w2, b2, geglu=True), eng.op_linear_ex(x, w2, b2, act=R.ACT_GEGLU)[0])
    xc = g.standard_normal((2, 64, 8, 8), dtype=np.float32)
    wc = (g.standard_normal((128, 64, 3, 3), dtype=np.float32) / 24).astype(np.float32)
    bc = g.standard_normal(128, dtype=np.float32) * 0.1
    rc = g.standard_normal((2, 128, 8, 8), dtype=np.float32)
    assert np.array_equal(eng.op_conv2d(xc, wc, bc, silu=True), eng.op_conv2d_ex(xc, wc, bc, act=R.ACT_SILU))
    assert np.array_equal(eng.op_conv2d(xc, wc, bc, residual=rc, scale=0.75, stream_out=True),
                          eng.op_conv2d_ex(xc, wc, bc, residual=rc, scale=0.75, stream_out=True))


# ------------------------------------------------------------------------------------------------ convolutions
@functools.lru_cache(maxsize=None)
def conv_inputs(storage, B, Cin, H, Cout, ups):
    """per_sample: every sample's time-embedding row has an offset and a slope of its own of several units"""
    g = np.random.default_rng(7 * B + Cin + 3 * H + Cout)
    x = R.round_like(g.standard_normal((B, Cin, H, H)), storage)
    w = R.round_like(g.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(Cin * 9), storage)
    b = (0.1 * g.standard_normal(Cout)).astype(np.float32)
    smp, n = np.arange(B)[:, None], np.arange(Cout)[None, :]
    rowvec = (2.0 * ((smp % 5) + 1) * np.where(smp % 2, -1.0, 1.0) + 3.0 * ((smp % 3) + 1) * n / Cout).astype(np.float32)
    Ho = 2 * H if ups else H
    res = R.round_like(g.standard_normal((B, Cout, Ho, Ho)), storage)
    for a in (x, w, b, rowvec, res):
        a.setflags(write=False)
    return x, w, b, rowvec, res


@functools.lru_cache(maxsize=None)
def conv_products(storage, shape):
    x, w = conv_inputs(storage, *shape)[:2]
    return R.conv_products(np.repeat(np.repeat(x, 2, axis=2), 2, axis=3) if shape[4] else x, w)


def conv_expect(mode, shape, act, with_res, splitk):
    _, _, b, rowvec, res = conv_inputs(R.STORAGE[mode], *shape)
    return R.conv_ref_bound(mode, conv_products(R.STORAGE[mode], shape), b, rowvec, res if with_res else None, act, 0.75 if with_res else 1.0,
                            R.STORAGE[mode], splitk)


def run_conv(eng, what, shape, opts, family, splitk, acts):
    """rowvec (+ scale + residual into the stream) and each activation of `acts` on one conv shape under one option setting"""
    x, w, b, rowvec, res = conv_inputs(R.STORAGE[eng.mode], *shape)
    worst = 0.0
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        for act, with_res in [(a, False) for a in acts] + [(R.ACT_NONE, True)]:
            got = eng.op_conv2d_ex(x, w, b, residual=res if with_res else None, rowvec=rowvec, upsample=shape[4], act=act,
                                   scale=0.75 if with_res else 1.0, stream_out=with_res)
            ran = (eng.stat("gemm_family"), eng.stat("gemm_splitk"))
            ok = ran == (family, splitk) if splitk else (ran[0] == family and ran[1] >= 2)      # splitk 0: split, in as many slices as the mode's chunks give
            assert ok, f"{what} {shape} {opts} act {act}: ran (family, slices) {ran}, this case is about {(family, splitk or '>= 2')}"
            ref, bound = conv_expect(eng.mode, shape, act, with_res, ran[1])
            r = float((np.abs(got - ref) / bound).max()) if np.isfinite(got).all() else float("inf")
            worst = max(worst, r)
            assert r <= 1.0, f"{eng.mode} {what} {shape} {opts} act {act} residual {with_res}: err / bound {r:.3f}"
    finally:
        for k, v in {**PATCH_DEFAULTS, **GEMM_DEFAULTS}.items():
            eng.set_option(k, v)
    print(f"[gemm] conv {what} {eng.mode} family {family} splitk {splitk} {shape}: worst err / bound {worst:.3f}")


def test_conv_rowvec_and_relu_igemm(eng):
    run_conv(eng, "igemm", (2, 64, 8, 128, False), {"gemm_splitk": 1}, IGEMM, 1, (R.ACT_NONE, R.ACT_SILU, R.ACT_RELU))
    run_conv(eng, "igemm split-K", (3, 320, 16, 320, False), {"gemm_splitk": 4}, IGEMM, 4, (R.ACT_NONE, R.ACT_RELU))


@pytest.mark.parametrize("shape,settings", [((24, 128, 32, 164, False), PATCH_UNSPLIT), ((48, 64, 16, 96, True), PATCH_UNSPLIT),
                                            ((2, 576, 16, 168, False), PATCH_SPLIT)])
def test_conv_rowvec_and_relu_patch(eng, shape, settings):
    """ReLU runs where the family has it: the first two generations on a conv without the fused upsample (with it, SiLU stands in for the
    activation slot); the 4-wave generation has no activation at all, and the dispatch must send a ReLU conv elsewhere."""
    for opts, family in settings:
        family = family if eng.two_byte else PATCH1
        split = 0 if settings is PATCH_SPLIT else 1
        if family != PATCH4:
            run_conv(eng, "patch", shape, opts, family, split, (R.ACT_NONE, R.ACT_SILU if shape[4] else R.ACT_RELU))
            continue
        run_conv(eng, "patch", shape, opts, PATCH4, 1, (R.ACT_NONE,))
        x, w, b, rowvec, _ = conv_inputs(R.STORAGE[eng.mode], *shape)
        try:
            for k, v in opts.items():
                eng.set_option(k, v)
            got = eng.op_conv2d_ex(x, w, b, rowvec=rowvec, upsample=shape[4], act=R.ACT_RELU)
            ran = eng.stat("gemm_family")
        finally:
            for k, v in PATCH_DEFAULTS.items():
                eng.set_option(k, v)
        assert ran in (PATCH1, PATCH2, IGEMM), f"{shape} {opts}: a ReLU conv ran on family {ran}; the 4-wave patch conv has no activation"
        ref, bound = conv_expect(eng.mode, shape, R.ACT_RELU, False, 1)
        r = float((np.abs(got - ref) / bound).max())
        print(f"[gemm] conv ReLU under {opts} {eng.mode} went to family {ran} {shape}: worst err / bound {r:.3f}")
        assert r <= 1.0


# ------------------------------------------------------------------------------------------------ refusals
def test_refuses_what_the_kernels_do_not_launch(eng):
    """A combination no kernel computes is an error of the hook, never another kernel's result or a silently dropped operand."""
    g = np.random.default_rng(9)
    x = g.standard_normal((300, 1280), dtype=np.float32)
    w = (g.standard_normal((320, 1280), dtype=np.float32) / 36).astype(np.float32)
    w2 = (g.standard_normal((640, 1280), dtype=np.float32) / 36).astype(np.float32)
    row = g.standard_normal((3, 320), dtype=np.float32)
    ones = np.ones(1280, np.float32)

    def refused(what, fn, **opts):
        try:
            for k, v in opts.items():
                eng.set_option(k, v)
            with pytest.raises(E.PdError):
                fn()
                pytest.fail(f"{eng.mode}: {what} was not refused", pytrace=False)
        finally:
            for k, v in GEMM_DEFAULTS.items():
                eng.set_option(k, v)

    refused("split-K with a V^T side output", lambda: eng.op_linear_ex(x, w, rows_per_sample=100, vt_begin=160), gemm_splitk=4, ring=0)
    refused("split-K GEGLU", lambda: eng.op_linear_ex(x, w2, act=R.ACT_GEGLU), gemm_splitk=4, ring=0)
    refused("split-K gated tanh-GELU", lambda: eng.op_linear_ex(x, w2, act=R.ACT_GATED), gemm_splitk=4, ring=0)
    refused("gate with a LayerNorm fold", lambda: eng.op_linear_ex(x, w, rows_per_sample=100, gate=row, ln=(ones, ones)), ring=0)
    refused("row remap with a LayerNorm fold", lambda: eng.op_linear_ex(x, w, rows_per_sample=100, c_sample_rows=133, c_row_off=33, ln=(ones, ones)), ring=0)
    refused("vt_begin that is no multiple of 4", lambda: eng.op_linear_ex(x, w, rows_per_sample=100, vt_begin=162))
    refused("N % 4 != 0 with a per-sample row", lambda: eng.op_linear_ex(x, w[:318], rows_per_sample=100, rowvec=row[:, :318]))
    refused("a gate on a GEGLU layer", lambda: eng.op_linear_ex(x, w2, act=R.ACT_GEGLU, rows_per_sample=100, gate=row))
    refused("a gate on a ReLU layer", lambda: eng.op_linear_ex(x, w, act=R.ACT_RELU, rows_per_sample=100, gate=row))
    refused("vt_tok_off outside the MM instantiations", lambda: eng.op_linear_ex(x, w, rows_per_sample=100, vt_begin=160, vt_tok_off=33))
    # a forced tile the launcher would replace by another one is an error, not that other tile's result
    if eng.two_byte:
        refused("tile 3 with a gate", lambda: eng.op_linear_ex(x[:, :320], w[:, :320], rows_per_sample=100, gate=row), gemm_tile=3, gemm_splitk=1, ring=0)
        refused("tile 3 with tanh-GELU", lambda: eng.op_linear_ex(x[:, :320], w[:, :320], act=R.ACT_TANH), gemm_tile=3, gemm_splitk=1, ring=0)
        refused("tile 3 on a split launch", lambda: eng.op_linear_ex(x, w), gemm_tile=3, gemm_splitk=4, ring=0)
    else:
        for t in (2, 3, 4):
            refused(f"tile {t} in an fp32-storage mode", lambda: eng.op_linear_ex(x[:, :320], w[:, :320]), gemm_tile=t, gemm_splitk=1)
    if eng.two_byte:     # the 256 x 192 tile exists for linear layers over 2-byte operands only, and only they convert an fp32 A while staging
        refused("a row remap under an fp32 A", lambda: eng.op_linear_ex(x, w, a_silu=True, rows_per_sample=100, c_sample_rows=133, c_row_off=33), ring=0)
        xc = g.standard_normal((2, 64, 8, 8), dtype=np.float32)
        wc = (g.standard_normal((192, 64, 3, 3), dtype=np.float32) / 24).astype(np.float32)
        refused("tile 4 on a conv", lambda: eng.op_conv2d_ex(xc, wc), gemm_tile=4, gemm_splitk=1)
        refused("tile 4 on an fp32 A", lambda: eng.op_linear_ex(x, w, a_silu=True), gemm_tile=4, gemm_splitk=1, ring=0)
    # and the engine still works after a refusal
    y, _, touched = eng.op_linear_ex(x[:, :200], w[:, :200])
    assert np.isfinite(y).all() and touched == 0
