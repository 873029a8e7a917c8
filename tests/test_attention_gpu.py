"""Every instantiation of the attention kernels against fp64, per element (tests/attn_ref.py holds the reference, the input families and
the bound; tests/test_attn_ref_cpu.py shows that the bound has teeth).

attention.hip through pd_op_attention_ex, in the forms the engine launches and pd_op_attention cannot express: q | k as column slices
of one buffer with row stride 2C and explicit sample strides (Nq < Nk included: the output rows past Nq belong to someone else), any
head count (dh 8 .. 160), causal mask, relative-position bias, a scale of the caller's, V^T pad columns full of NaN.  In the 2-byte
modes every case runs twice, on attn2_kernel (by nature) and on attn_kernel (option attn_legacy); every case asserts stat
"attn_kernel", so a case that moves to the other kernel fails instead of passing on the wrong code.  vae_attention.hip through
pd_op_vae_attention under the same bound with one head.

Each test prints its worst err / bound ("[attn] ..." lines, pytest -s)."""
import collections
import functools

import numpy as np
import pytest

from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import weights as W
from tests import attn_ref as R
from tests.test_sd3_vae_attention_gpu import SHAPES as VAE_SHAPES

pytestmark = pytest.mark.gpu

GENERIC, PIPELINED = 1, 2          # PD_ATTN_* of include/pdengine.h
KNAME = {GENERIC: "attn_kernel", PIPELINED: "attn2_kernel"}
NAN = float("nan")
DHS = [8, 16, 32, 40, 64, 80, 160]

Case = collections.namedtuple("Case", "family B Nq Nk heads dh causal bias scale layout vt_extra pad_fill", defaults=(False, False, 0.0, 0, 0, 0.0))


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
def inputs(storage, c):
    """inputs and reference of a case, shared by the modes of one storage type and by both kernels; never modified"""
    mode = {"f32": "f32", "f16": "f16", "bf16": "bf16"}[storage]
    seed = 1000 * R.FAMILIES.index(c.family) + 97 * c.B + 13 * c.Nq + 7 * c.Nk + 3 * c.heads + c.dh + (500 if c.causal else 0)
    q, k, v = R.make_inputs(c.family, seed, c.B, c.Nq, c.Nk, c.heads, c.dh, mode, c.scale)
    rb = R.make_relbias(seed + 1, c.heads, c.Nk) if c.bias else None
    ref, _, s = R.attention_ref(q, k, v, c.heads, c.scale, c.causal, rb, want_logits=True)
    if c.family == "staircase" and c.Nk > 2 * R.TK:    # the inputs do what the family is for: one rise below the lazy threshold, one above
        (lo1, hi1), (lo2, hi2) = R.staircase_rises(s)
        assert 6.0 < lo1 and hi1 < R.LAZY_THR < lo2 and hi2 < 10.0, (c, lo1, hi1, lo2, hi2)
    for a in (q, k, v, ref):
        a.setflags(write=False)
    return q, k, v, rb, ref


@functools.lru_cache(maxsize=None)
def bound_of(mode, c):
    q, k, v, rb, ref = inputs(R.STORAGE[mode], c)
    b = R.attention_bound(mode, q, k, v, c.heads, c.scale, c.causal, rb)
    b.setflags(write=False)
    return b


def run_cases(eng, what, cases):
    """Every case on every kernel family the mode has for it; prints the worst err / bound per family, fails with every case past it."""
    worst, fails = {}, []
    for c in cases:
        q, k, v, rb, ref = inputs(R.STORAGE[eng.mode], c)
        bound = bound_of(eng.mode, c)
        natural = PIPELINED if eng.two_byte and not c.causal and not c.bias else GENERIC
        for legacy, want in ([(0, natural)] + ([(1, GENERIC)] if natural == PIPELINED else [])):
            eng.set_option("attn_legacy", legacy)
            try:
                got, touched = eng.op_attention_ex(q, k, v, heads=c.heads, causal=c.causal, scale=c.scale, relbias=rb, layout=c.layout,
                                                   vt_extra=c.vt_extra, pad_fill=c.pad_fill)
                ran = eng.stat("attn_kernel")
            finally:
                eng.set_option("attn_legacy", 0)
            assert ran == want, f"{c}: ran {KNAME.get(ran, ran)}, this case is about {KNAME[want]}"
            assert touched == 0, f"{c} on {KNAME[want]}: {touched} elements of the output rows >= Nq changed"
            r, at = R.check(got, ref, bound)
            if r > worst.get(want, (0.0,))[0]:
                worst[want] = (r, c, at)
            if not r <= 1.0:
                fails.append((KNAME[want], c, r, at))
    for kern, (r, c, at) in sorted(worst.items()):
        print(f"[attn] {what} {eng.mode} {KNAME[kern]}: worst err / bound {r:.3f} at {at} of {c}")
    assert not fails, f"{eng.mode} {what}: err / bound > 1 in {len(fails)} runs: " + "; ".join(
        f"{kn} {c} {r:.3f} at (b, query, channel) {at}" for kn, c, r, at in fails[:6])


def instantiation_cases(dh):
    """Two heads.  Every Nk of {1, 8, 63, 64, 65, 77, 128, 129, 200} and every Nq of {1, 17, 33, 128, 130}; every family at Nk 65 and 200;
    layout 1 with NaN fills at Nq == Nk and Nq < Nk, vt_extra 0 and 8; layout 0 with NaN pads wherever Nk is no multiple of 8; B = 2."""
    c = [Case("normal", 1, 1, 1, 2, dh, pad_fill=NAN),
         Case("normal", 1, 17, 8, 2, dh),
         Case("peaked", 1, 33, 63, 2, dh, pad_fill=NAN),
         Case("flat", 1, 128, 64, 2, dh),
         Case("negative", 2, 33, 77, 2, dh, layout=1, vt_extra=8, pad_fill=NAN),
         Case("peaked", 1, 77, 77, 2, dh, layout=1, pad_fill=NAN),
         Case("normal", 1, 130, 128, 2, dh, vt_extra=8, pad_fill=NAN),
         Case("staircase", 1, 130, 129, 2, dh, pad_fill=NAN),
         Case("negative", 1, 128, 129, 2, dh, layout=1, pad_fill=NAN)]
    for i, fam in enumerate(("normal", "flat", "negative", "peaked", "staircase", "large")):
        c.append(Case(fam, 1, (17, 33)[i % 2], 65, 2, dh, pad_fill=NAN))
        c.append(Case(fam, 2 if fam == "negative" else 1, (33, 17, 130)[i % 3], 200, 2, dh, layout=1 if fam == "peaked" else 0, vt_extra=8 * (i % 2),
                      pad_fill=NAN))
    if dh in (40, 64):     # 17 tiles: long accumulation, many rescales
        c += [Case("negative", 1, 17, 1029, 2, dh, pad_fill=NAN), Case("peaked", 1, 33, 1029, 2, dh, pad_fill=NAN)]
    return c


def test_case_list_covers_what_it_claims():
    for dh in DHS:
        cs = instantiation_cases(dh)
        assert {c.Nk for c in cs} >= {1, 8, 63, 64, 65, 77, 128, 129, 200} and {c.Nq for c in cs} == {1, 17, 33, 77, 128, 130}
        for nk in (65, 200):
            assert {c.family for c in cs if c.Nk == nk} == {"normal", "flat", "negative", "peaked", "staircase", "large"}
        l1 = [c for c in cs if c.layout == 1]
        assert any(c.Nq == c.Nk for c in l1) and any(c.Nq < c.Nk for c in l1) and {c.vt_extra for c in l1} == {0, 8}
        assert all(np.isnan(c.pad_fill) for c in l1) and any(c.B == 2 for c in cs)
        assert any(c.layout == 0 and np.isnan(c.pad_fill) and c.Nk % 8 for c in cs)
        assert any(c.family == "staircase" and c.Nk >= 129 for c in cs)


@pytest.mark.parametrize("dh", DHS)
def test_instantiations(eng, dh):
    run_cases(eng, f"dh {dh}", instantiation_cases(dh))


def test_causal(eng):
    """Row 0 sees one key, the last rows all; attn_kernel in every mode (the pipelined kernel has no mask)."""
    cases = [Case(fam, 1, n, n, heads, 64, causal=True, pad_fill=NAN)
             for heads in (2, 3) for n in (1, 63, 65, 77, 130) for fam in ("normal", "negative", "peaked")]
    cases += [Case(fam, 2, n, n, 2, 40, causal=True, layout=1, pad_fill=NAN) for n, fam in ((65, "normal"), (77, "negative"), (130, "peaked"))]
    run_cases(eng, "causal", cases)


def test_relative_position_bias(eng):
    """T5's form: scale 1, bias rows with a slope of their own per head (a shifted index or the neighbouring head's row shows)."""
    cases = [Case(fam, 1, n, n, heads, 64, bias=True, scale=1.0, pad_fill=NAN)
             for heads in (2, 3) for n in (1, 63, 65, 77, 130) for fam in ("flat", "normal")]
    cases.append(Case("flat", 2, 77, 77, 2, 64, bias=True, scale=1.0, layout=1, pad_fill=NAN))
    run_cases(eng, "bias", cases)


def test_scale_argument(eng):
    run_cases(eng, "scale 0.5", [Case("normal", 1, 33, 77, 2, 64, scale=0.5), Case("large", 1, 17, 65, 2, 40, scale=0.125)])


def test_plain_hook_is_the_extended_one_at_its_defaults(eng):
    g = np.random.default_rng(5)
    C = 8 * 40
    q, k, v = (R.round_like(g.standard_normal(s, dtype=np.float32), eng.mode) for s in ((2, 40, C), (2, 77, C), (2, 77, C)))
    a = eng.op_attention(q, k, v)
    b, touched = eng.op_attention_ex(q, k, v)
    assert np.array_equal(a, b) and touched == 0
    assert eng.stat("attn_kernel") == (PIPELINED if eng.two_byte else GENERIC)


def test_refuses_what_the_engine_does_not_launch(eng):
    """Not a fall-back: bias with dh != 64, with Nq != Nk, with the causal mask; the causal mask with Nq != Nk; a head dim without a
    kernel; layout 1 with more queries than keys."""
    z = lambda n, c: np.zeros((1, n, c), np.float32)
    rb = lambda h, n: np.zeros((h, 2 * n - 1), np.float32)
    for kw, (nq, nk, c) in [(dict(heads=2, relbias=rb(2, 16)), (16, 16, 80)),
                            (dict(heads=2, relbias=rb(2, 24)), (16, 24, 128)),
                            (dict(heads=2, relbias=rb(2, 16), causal=True), (16, 16, 128)),
                            (dict(heads=2, causal=True), (16, 24, 128)),
                            (dict(heads=2), (16, 16, 48)),
                            (dict(heads=2, layout=1), (24, 16, 128)),
                            (dict(heads=2, vt_extra=4), (16, 16, 128))]:
        with pytest.raises(E.PdError):
            eng.op_attention_ex(z(nq, c), z(nk, c), z(nk, c), **kw)


def test_vae_attention(eng2):
    """vae_attention.hip (one head over all channels) under the same per-element bound: the shapes of test_sd3_vae_attention_gpu.py on
    N(0, 1) inputs, and the families that show a pad key counted or the last key dropped."""
    eng = eng2
    cases = [Case("normal", B, N, N, 1, C) for B, N, C in VAE_SHAPES]
    cases += [Case(fam, B, N, N, 1, C) for fam in ("negative", "peaked_last") for B, N, C in ((1, 40, 512), (2, 240, 128))]
    worst, fails = (0.0, None, None), []
    eng.set_option("vae_flash", 1)
    try:
        for c in cases:
            q, k, v, _, ref = inputs(R.STORAGE[eng.mode], c)
            n0 = eng.stat("vae_flash_launches")
            got = eng.op_vae_attention(q, k, v)
            assert eng.stat("vae_flash_launches") == n0 + 1
            r, at = R.check(got, ref, bound_of(eng.mode, c))
            if r > worst[0]:
                worst = (r, c, at)
            if not r <= 1.0:
                fails.append((c, r, at))
    finally:
        eng.set_option("vae_flash", -1)
    print(f"[attn] vae {eng.mode} vae_attn_kernel: worst err / bound {worst[0]:.3f} at {worst[2]} of {worst[1]}")
    assert not fails, fails
