"""The attention bound of tests/attn_ref.py has teeth: mistakes a kernel could make, applied to the fp64 reference itself, exceed it
by a factor of at least 4 on some element in both 2-byte modes, on the input family built to show them -- while the reference with
nothing but its output rounded to the compute type stays below 1.  No GPU, no engine.

On N(0, 1) inputs a bf16 bound cannot see one key too many or too few (`drop_last` on `normal` stays near 4, `pad_key` on `flat` near
1), which is why test_attention_gpu.py runs the families below and not only `normal`."""
import functools

import numpy as np
import pytest

from tests import attn_ref as R

MODES2 = ("bf16", "f16")
FACTOR = 4.0
# (Nq, Nk, dh), two heads each: one ragged tile of one key, a ragged second tile, three tiles with a single key in the last, four tiles
SHAPES = [(33, 65, 64), (33, 77, 16), (17, 129, 40), (33, 200, 64)]
# mutant -> (family that covers it, what attention_ref needs besides q, k, v)
COVER = [("drop_last", "peaked_last", {}),
         ("pad_key", "negative", {}),
         ("causal_off1", "normal", {"causal": True}),
         ("causal_off1", "negative", {"causal": True}),
         ("bias_off1", "flat", {"bias": True, "scale": 1.0}),
         ("bias_next_head", "flat", {"bias": True, "scale": 1.0}),
         ("k_next_head", "normal", {}),
         ("no_log2e", "normal", {}),
         ("v_swap", "peaked_last", {}),
         ("stale_alpha", "staircase", {}),
         ("stale_alpha", "peaked", {})]


@functools.lru_cache(maxsize=None)
def case(mode, family, shape, causal=False, bias=False, scale=None):
    Nq, Nk, dh = shape
    if causal or bias:
        Nq = Nk
    if bias:
        dh = 64
    q, k, v = R.make_inputs(family, 100 + Nk + dh, 1, Nq, Nk, 2, dh, mode, scale)
    rb = R.make_relbias(7 + Nk, 2, Nk) if bias else None
    ref, _ = R.attention_ref(q, k, v, 2, scale, causal, rb)
    bound = R.attention_bound(mode, q, k, v, 2, scale, causal, rb)
    return q, k, v, rb, ref, bound


def test_every_mutant_is_covered():
    assert {m for m, _, _ in COVER} == set(R.MUTANTS)


@pytest.mark.parametrize("mode", MODES2)
@pytest.mark.parametrize("mutant,family,kw", COVER, ids=[f"{m}-{f}" for m, f, _ in COVER])
def test_mutant_exceeds_bound(mode, mutant, family, kw):
    """Past the bound at every shape, and by the factor at one of them at least."""
    worst = []
    for shape in SHAPES:
        q, k, v, rb, ref, bound = case(mode, family, shape, **kw)
        got, _ = R.attention_ref(q, k, v, 2, kw.get("scale"), kw.get("causal", False), rb, mutant=mutant)
        r, at = R.check(got, ref, bound)
        print(f"[attn-teeth] {mode} {mutant} on {family} {shape}: err / bound {r:.1f} at {at}")
        assert r > 1.0, (mutant, family, shape, r)
        worst.append(r)
    assert max(worst) >= FACTOR, (mutant, family, worst)


@pytest.mark.parametrize("mode", MODES2)
def test_output_rounding_alone_meets_bound(mode):
    seen = set()
    for _, family, kw in COVER:
        for shape in SHAPES:
            key = (family, shape, tuple(sorted(kw.items())))
            if key in seen:
                continue
            seen.add(key)
            q, k, v, rb, ref, bound = case(mode, family, shape, **kw)
            r, at = R.check(R.round_like(ref.astype(np.float32), mode), ref, bound)
            assert r < 1.0, (family, shape, r, at)


def test_flat_carries_f16_only():
    """`flat` (v off centre, nearly uniform weights) shows a normalisation mistake of 1 / Nk against a bound of about 2 u: enough in
    f16 at short rows, not in bf16 -- `negative` carries the pad-key mutant there."""
    for shape in SHAPES[:2]:
        q, k, v, rb, ref, bound = case("f16", "flat", shape)
        got, _ = R.attention_ref(q, k, v, 2, mutant="pad_key")
        assert R.check(got, ref, bound)[0] >= FACTOR


@pytest.mark.parametrize("mode", ("f32",) + MODES2)
@pytest.mark.parametrize("dh", [8, 16, 32, 40, 64, 80, 160])
def test_staircase_steps_straddle_the_lazy_threshold(mode, dh):
    """The row maximum rises by less than LAZY_THR from tile 0 to tile 1 and by more from tile 1 to tile 2, in every row."""
    for Nq, Nk in [(33, 129), (130, 200)]:
        q, k, v = R.make_inputs("staircase", 5 + dh, 1, Nq, Nk, 2, dh, mode)
        _, _, s = R.attention_ref(q, k, v, 2, want_logits=True)
        (lo1, hi1), (lo2, hi2) = R.staircase_rises(s)
        print(f"[attn-teeth] staircase {mode} dh {dh} Nk {Nk}: rises {lo1:.2f} .. {hi1:.2f}, {lo2:.2f} .. {hi2:.2f}")
        assert 6.0 < lo1 and hi1 < R.LAZY_THR, (lo1, hi1)
        assert R.LAZY_THR < lo2 and hi2 < 10.0, (lo2, hi2)


def test_peaked_keys_sit_on_the_tile_edges():
    assert R.peaked_positions(200) == [5, 63, 64, 199] and R.peaked_positions(65) == [5, 63, 64] and R.peaked_positions(1) == [0]
    q, k, v = R.make_inputs("peaked", 3, 1, 17, 77, 2, 64, "bf16")
    _, p = R.attention_ref(q, k, v, 2)
    for kp in R.peaked_positions(77):
        assert p[0, :, :, kp].max() > 0.9
