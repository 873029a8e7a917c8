"""The upsample-conv fold on the host (tests/upfold_ref.py): the four phase convs equal conv3x3(repeat2(x)), borders included."""
import numpy as np
import pytest

from tests import upfold_ref as R

SHAPES = [(2, 8, 4, 4, 8), (1, 5, 3, 7, 6), (3, 13, 6, 2, 3), (1, 1, 1, 1, 1), (2, 7, 1, 5, 4)]   # B, Cin, H, W, Cout


@pytest.mark.parametrize("B,Cin,H,W,Cout", SHAPES)
def test_phase_convs_equal_upsampled_conv_float64(B, Cin, H, W, Cout):
    g = np.random.default_rng(B * 1000 + Cin * 10 + H)
    x = g.standard_normal((B, Cin, H, W))
    w = g.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9 * Cin)
    b = g.standard_normal(Cout)
    ref = R.conv3x3_same(R.repeat2(x), w, b)
    got = R.phase_convs(x, R.fold_weights(w), b)
    assert got.shape == ref.shape == (B, Cout, 2 * H, 2 * W)
    assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("B,Cin,H,W,Cout", SHAPES)
def test_phase_convs_exact_on_integers(B, Cin, H, W, Cout):
    g = np.random.default_rng(7 + Cin)
    x = g.integers(-3, 4, (B, Cin, H, W)).astype(np.float64)
    w = g.integers(-2, 3, (Cout, Cin, 3, 3)).astype(np.float64)
    b = g.integers(-4, 5, Cout).astype(np.float64)
    np.testing.assert_array_equal(R.phase_convs(x, R.fold_weights(w), b), R.conv3x3_same(R.repeat2(x), w, b))


def test_fold_sets():
    """every original tap lands in exactly one folded tap of every phase, and a phase's four taps carry all nine"""
    w = np.arange(9, dtype=np.float64).reshape(1, 1, 3, 3) + 1
    wf = R.fold_weights(w)
    assert wf.shape == (4, 1, 1, 2, 2)
    for ph in range(4):
        assert wf[ph].sum() == w.sum()
    np.testing.assert_array_equal(wf[0, 0, 0], [[1, 2 + 3], [4 + 7, 5 + 6 + 8 + 9]])
    np.testing.assert_array_equal(wf[3, 0, 0], [[1 + 2 + 4 + 5, 3 + 6], [7 + 8, 9]])
