"""tests/canny_ref.py (the NumPy restatement of cv2.Canny that the engine's kernels are held to) against hand-derived cases: the
properties of the algorithm that can go wrong silently.  No engine, no GPU."""
import numpy as np
import pytest

from tests import canny_ref as R


def step_picture():
    img = np.zeros((8, 8), np.uint8)
    img[:, 4:] = 255
    return img


def test_vertical_step_keeps_one_column():
    """0 | 255 between columns 3 and 4: both columns have m = 4 * 255 = 1020, dy = 0 -> horizontal class; column 3 passes
    m > m[0,-1] = 0 and m >= m[0,+1] = 1020, column 4 fails m > m[0,-1] = 1020.  Replicated borders: rows 0 and 7 as the others."""
    img = step_picture()
    dx, dy, m = R.gradients(img)
    assert (m[:, 3] == 1020).all() and (m[:, 4] == 1020).all() and (dy == 0).all()
    assert (np.delete(m, [3, 4], axis=1) == 0).all()
    want = np.zeros((8, 8), np.uint8)
    want[:, 3] = 255
    assert np.array_equal(R.canny(img, 100, 200), want)
    assert np.array_equal(R.canny_states(img, 100, 200), want // 255 * R.STRONG)


def test_horizontal_step_keeps_one_row():
    img = step_picture().T.copy()
    dx, dy, m = R.gradients(img)
    assert (m[3] == 1020).all() and (m[4] == 1020).all() and (dx == 0).all()
    want = np.zeros((8, 8), np.uint8)
    want[3] = 255
    assert np.array_equal(R.canny(img, 100, 200), want)


def test_three_channel_step_equals_grey():
    img = step_picture()
    assert np.array_equal(R.canny(np.stack([img] * 3, axis=2), 100, 200), R.canny(img, 100, 200))


def test_thresholds_are_floored_and_swapped():
    img = R.blobs(37, 53, 3, B=1, seed=1)[0]
    assert np.array_equal(R.canny_states(img, 100.9, 200.9), R.canny_states(img, 100, 200))
    step = np.zeros((8, 8), np.uint8)
    step[:, 4:] = 50                      # m = 200 in column 3: rounding 199.9 up to 200 would change its state
    assert (R.canny_states(step, 100, 199.9)[:, 3] == R.STRONG).all()
    assert (R.canny_states(step, 199.9, 300)[:, 3] == R.WEAK).all()
    assert np.array_equal(R.canny(img, 200, 100), R.canny(img, 100, 200))
    assert np.array_equal(R.canny_states(img, 200, 100), R.canny_states(img, 100, 200))


def test_thresholds_are_strict():
    """a step of height v between columns 3 and 4 has m = 4 v in column 3, the only candidate column"""
    img = np.zeros((8, 8), np.uint8)
    img[:, 4:] = 50                       # m = 200
    col = lambda lo, hi: R.canny_states(img, lo, hi)[:, 3]
    assert (col(100, 200) == R.WEAK).all()      # m == hi: not strong
    assert (col(100, 199) == R.STRONG).all()
    assert (col(200, 300) == R.NONE).all()      # m == lo: not a candidate
    assert (col(199, 300) == R.WEAK).all()
    assert not R.canny(img, 100, 200).any()     # weak only: nothing survives


def test_channel_select_largest_magnitude_lowest_index_on_ties():
    v = np.zeros((8, 8), np.uint8)
    v[:, 4:] = 100                               # vertical step: dx = 400, dy = 0
    h = np.zeros((8, 8), np.uint8)
    h[4:, :] = 100                               # horizontal step: dx = 0, dy = 400
    h_big = (h.astype(np.int32) * 2).astype(np.uint8)
    z = np.zeros((8, 8), np.uint8)
    # at (1, 3) only the vertical step has a gradient, at (3, 1) only the horizontal one
    dx, dy, m = R.gradients(np.stack([z, v, h], axis=2))
    assert (dx[1, 3], dy[1, 3], m[1, 3]) == (400, 0, 400) and (dx[3, 1], dy[3, 1], m[3, 1]) == (0, 400, 400)
    # at (3, 3) both have n = 400: the tie goes to the lower channel index, whichever picture sits there
    dx, dy, m = R.gradients(np.stack([z, v, h], axis=2))
    assert (dx[3, 3], dy[3, 3], m[3, 3]) == (400, 0, 400)
    dx, dy, m = R.gradients(np.stack([z, h, v], axis=2))
    assert (dx[3, 3], dy[3, 3], m[3, 3]) == (0, 400, 400)
    # a strictly larger n in a later channel wins
    dx, dy, m = R.gradients(np.stack([v, z, h_big], axis=2))
    assert (dx[3, 3], dy[3, 3], m[3, 3]) == (0, 800, 800)


def test_hysteresis_follows_diagonals_and_drops_orphans():
    st = np.zeros((9, 9), np.uint8)
    st[0, 0] = R.STRONG
    for i in range(1, 6):
        st[i, i] = R.WEAK                        # a diagonal chain off the strong pixel: 8-connected only
    st[7, 0:3] = R.WEAK                          # a weak component with no strong pixel; (6, 1) would join it to nothing
    st[2, 7] = R.WEAK                            # an isolated weak pixel
    out = R.hysteresis(st)
    want = st.copy()
    for i in range(1, 6):
        want[i, i] = R.STRONG
    assert np.array_equal(out, want)
    assert (st[0, 0], st[1, 1]) == (R.STRONG, R.WEAK)   # the input is left alone
    # a gap of one pixel breaks the chain
    st2 = st.copy()
    st2[3, 3] = R.NONE
    out2 = R.hysteresis(st2)
    assert out2[2, 2] == R.STRONG and out2[4, 4] == R.WEAK and out2[5, 5] == R.WEAK


def test_hysteresis_agrees_with_connected_components():
    ndimage = pytest.importorskip("scipy.ndimage")
    img = R.blobs(64, 64, 3, B=1, seed=2)[0]
    st = R.canny_states(img, 100, 200)
    lab, n = ndimage.label(st != R.NONE, structure=np.ones((3, 3)))
    ok = np.zeros(n + 1, bool)
    ok[np.unique(lab[st == R.STRONG])] = True
    ok[0] = False
    assert np.array_equal(R.hysteresis(st) == R.STRONG, ok[lab])


def test_test_pictures_exercise_the_hysteresis():
    """the GPU tests' inputs: at (100, 200) every blob size has weak pixels that survive and weak pixels that are dropped; the spiral is
    one component hanging off its block and vanishes without it; the serpentine is one path"""
    for H, W in R.BLOB_SIZES:
        for C in (1, 3):
            st = np.stack([R.canny_states(img, 100, 200) for img in R.blobs(H, W, C)])
            out = np.stack([R.hysteresis(s) for s in st])
            kept, dropped = ((st == R.WEAK) & (out == R.STRONG)).sum(), ((st == R.WEAK) & (out == R.WEAK)).sum()
            print(f"blobs {H}x{W} C={C}: weak kept {kept}, weak dropped {dropped}")
            assert kept > 0 and dropped > 0, (H, W, C)
    sp = R.spiral()
    st = R.canny_states(sp, 100, 200)
    out = R.hysteresis(st)
    assert (st == R.STRONG).sum() > 0 and (out == R.STRONG).sum() == (st != R.NONE).sum() > 5000
    kept = (st == R.WEAK) & (out == R.STRONG)
    ys, xs = np.nonzero(kept)
    assert len(set(zip(ys // 64, xs // 64))) == 9          # the kept weak pixels touch every 64 x 64 cell
    assert not R.canny(R.spiral(block=30), 100, 200).any()
    s, path, seg = R.serpentine()
    out = R.hysteresis(s)
    assert (out[path] == R.STRONG).all() and (out[seg] == R.WEAK).all()


def test_matches_cv2_where_installed():
    cv2 = pytest.importorskip("cv2")
    for H, W in R.BLOB_SIZES:
        for C in (1, 3):
            for img in R.blobs(H, W, C):
                for lo, hi in R.BLOB_THRESHOLDS:
                    assert np.array_equal(cv2.Canny(np.ascontiguousarray(img if C == 3 else img[:, :, 0]), lo, hi), R.canny(img, lo, hi))
    for block in (255, 30):
        assert np.array_equal(cv2.Canny(R.spiral(block=block), 100, 200), R.canny(R.spiral(block=block), 100, 200))
