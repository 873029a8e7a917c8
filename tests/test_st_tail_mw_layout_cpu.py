"""Multi-window maps of the fused transformer tail (csrc/st_tail.hip, template parameter NW), checked on the CPU through
tests/st_tail_mw_emul.py: where every context K / V element lands, the order in which the ring delivers the fragments against the
order in which the kernel's phases consume them, and the online softmax across the windows against the plain formula."""
import numpy as np
import pytest

from tests import st_tail_emul as E1
from tests import st_tail_mw_emul as MW


@pytest.mark.parametrize("Nk", [1, 77, 96, 97, 192, 231, 288])
def test_every_kv_element_lands_in_exactly_one_slot(Nk):
    nw = MW.windows(Nk)
    seen = {"K": np.zeros((Nk, E1.C), np.int32), "V": np.zeros((Nk, E1.C), np.int32)}
    for pp in range(4):
        for w in range(nw):
            for F in range(MW.KV_PAIR):
                for lane in range(64):
                    for j in range(8):
                        src = MW.kv_source(pp, w, F, lane, j)
                        if src is None:
                            continue
                        assert 0 <= src[2] < E1.C and MW.KWIN * w <= src[1] < MW.KWIN * (w + 1)
                        if src[1] < Nk:
                            seen[src[0]][src[1], src[2]] += 1
    assert (seen["K"] == 1).all() and (seen["V"] == 1).all()


@pytest.mark.parametrize("nw", [1, 2, 3])
def test_ring_delivers_what_the_phases_consume(nw):
    """step s of the ring holds fragments step_src(s) .. + 19; concatenated over the steps that is the kernel's consumption order"""
    delivered = []
    for s in range(MW.steps_total(nw)):
        kind, f0 = MW.step_src(s, nw)
        delivered += [(kind, f0 + i) for i in range(MW.SF)]
    want = MW.consumed(nw)
    assert len(want) == MW.steps_total(nw) * MW.SF
    assert delivered == want
    # every weight fragment once, every K / V fragment of the sample once
    assert sorted(f for k, f in delivered if k == "w") == list(range(MW.WF_A + MW.WF_B + E1.NCHUNK * 60 + E1.NT * E1.KS))
    assert sorted(f for k, f in delivered if k == "kv") == list(range(4 * nw * MW.KV_PAIR))
    # the prefetch past the end re-reads the last step
    assert MW.step_src(MW.steps_total(nw) + 4, nw) == MW.step_src(MW.steps_total(nw) - 1, nw)


def test_one_window_is_the_single_window_kernel():
    assert MW.steps_pair(1) == 9 and MW.steps_total(1) == 176
    r = np.random.default_rng(2)
    for Nk in (5, 77, 96):
        K2, V2 = r.standard_normal((Nk, E1.C)), r.standard_normal((Nk, E1.C))
        a, b = MW.pack_kv(K2, V2, Nk), E1.pack_kv(K2, V2, Nk)
        assert a.shape == (4, 1, 60, 64, 8)
        np.testing.assert_array_equal(a[:, 0], b)


@pytest.mark.parametrize("Nk,boost", [(77, None), (97, None), (192, None), (231, None), (231, 3), (231, 228), (288, None)])
def test_online_softmax_over_windows_matches_the_formula(Nk, boost):
    """q of one head pair for a wave's 32 tokens against softmax(q k^T scale) v per head; `boost`: a key whose logit dominates,
    in the first / the last window (the running max moves there, everything before is rescaled)"""
    r = np.random.default_rng(Nk)
    pp, scale = 1, E1.DH ** -0.5
    K2, V2 = r.standard_normal((Nk, E1.C)), r.standard_normal((Nk, E1.C))
    q = r.standard_normal((32, 2, E1.DH))
    if boost is not None:
        K2[boost] *= 25.0
    # q as the kernel holds it: three 32-slot accumulator tiles, head hl in k16 steps 3 hl .. 3 hl + 2 (48 slots, 40 real)
    qacc = np.zeros((3, 64, 16))
    for tl in range(3):
        for lane in range(64):
            for reg in range(16):
                ksq = 2 * tl + (reg >> 3)
                hl, d = ksq // 3, 16 * (ksq % 3) + 8 * (lane >> 5) + (reg & 7)
                if d < E1.DH:
                    qacc[tl, lane, reg] = q[lane & 31, hl, d]
    qf = np.concatenate([E1.acc_to_bfrags(qacc[tl]) for tl in range(3)])
    of = MW.attention_pair(qf, MW.pack_kv(K2, V2, Nk)[pp], Nk, scale)
    for hl in range(2):
        hd = 2 * pp + hl
        s = q[:, hl] @ K2[:, hd * E1.DH:(hd + 1) * E1.DH].T * scale
        p = np.exp(s - s.max(axis=1, keepdims=True))
        ref = (p / p.sum(axis=1, keepdims=True)) @ V2[:, hd * E1.DH:(hd + 1) * E1.DH]       # [32][40]
        assert np.isfinite(ref).all()
        got = np.zeros((32, E1.DH))
        for ksl in range(3):
            for lane in range(64):
                for j in range(8):
                    d = 32 * (ksl >> 1) + 16 * (lane >> 5) + 8 * (ksl & 1) + j
                    if d < E1.DH:
                        got[lane & 31, d] = of[hl, ksl, lane, j]
        np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-12)
