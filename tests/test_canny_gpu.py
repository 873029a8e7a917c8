"""The Canny edge detector on the GPU (pd_canny, pd_op_canny_hysteresis, Engine.canny, annotators.CannyDetector) against the NumPy
restatement of cv2.Canny in tests/canny_ref.py.  Every step is integer arithmetic and the float form is single-rounding fp32, so every
comparison is np.array_equal: every byte, no tolerance, no exempt pixels."""
import ctypes as C

import numpy as np
import pytest

from prompt_diffusion_amd import annotators as A
from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import weights as W
from tests import canny_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25)


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(W.TINY, precision="f32")   # no weights: the detector has none
    yield e
    e.close()


_REF = {}


def blob_case(H, W_, Cc):
    """(pictures [3, H, W, C], {thresholds: reference edge maps [3, H, W]}); computed once per case"""
    key = (H, W_, Cc)
    if key not in _REF:
        img = R.blobs(H, W_, Cc)
        refs = {t: R.canny_batch(img, *t) for t in R.BLOB_THRESHOLDS}
        img.setflags(write=False)
        for r in refs.values():
            r.setflags(write=False)
        _REF[key] = (img, refs)
    return _REF[key]


def host(x):
    return x.cpu().numpy() if E._is_torch(x) else np.asarray(x)


@pytest.mark.parametrize("Cc", [3, 1])
@pytest.mark.parametrize("H,W_", R.BLOB_SIZES, ids=[f"{h}x{w}" for h, w in R.BLOB_SIZES])
def test_blobs_match_reference(eng, H, W_, Cc):
    img, refs = blob_case(H, W_, Cc)
    # the input is not degenerate: at (100, 200) the reference both keeps and drops weak pixels
    st = np.stack([R.canny_states(i, 100, 200) for i in img])
    ref = refs[(100, 200)]
    kept, dropped = ((st == R.WEAK) & (ref == 255)).sum(), ((st == R.WEAK) & (ref == 0)).sum()
    print(f"blobs {H}x{W_} C={Cc}: weak kept {kept}, weak dropped {dropped}")
    assert kept > 0 and dropped > 0
    for (lo, hi), ref in refs.items():
        got = eng.canny(img, lo, hi)
        assert got.dtype == np.uint8 and got.shape == ref.shape
        assert np.array_equal(got, ref), (lo, hi, int((got != ref).sum()))
        print(f"  thresholds ({lo}, {hi}): {int((ref == 255).sum())} edge pixels, {eng.stat('canny_sweeps')} sweeps")
    if Cc == 1:   # [B, H, W] is [B, H, W, 1]
        assert np.array_equal(eng.canny(img[:, :, :, 0], 100, 200), refs[(100, 200)])


@pytest.mark.parametrize("block", [255, 30])
def test_spiral_floods_across_every_tile(eng, block):
    """one component of > 5000 candidates hanging off the block's 44 strong pixels, through every 64 x 64 cell of the picture: a sweep
    loop that stops a launch early, or a halo that is not read again, loses its far end.  Without the block nothing is strong."""
    img = R.spiral(block=block)
    ref = R.canny(img, 100, 200)
    assert (ref == 255).sum() > 5000 if block == 255 else not ref.any()
    got = eng.canny(img[None], 100, 200)[0]
    print(f"spiral block={block}: {int((ref == 255).sum())} edge pixels, {eng.stat('canny_sweeps')} sweeps")
    assert np.array_equal(got, ref), int((got != ref).sum())
    if block == 255:   # the same bytes in a second run, and in a batch next to the picture that stays empty
        both = np.stack([img, R.spiral(block=30), img])
        got = eng.canny(both, 100, 200)
        assert np.array_equal(got[0], ref) and not got[1].any() and np.array_equal(got[2], ref)


def test_ops_hysteresis_serpentine(eng):
    import torch
    st, path, seg = R.serpentine()
    out = eng.canny_hysteresis(st[None])[0]
    print(f"serpentine: path of {int(path.sum())} pixels, {eng.stat('canny_sweeps')} sweeps")
    assert (out[path] == R.STRONG).all() and (out[seg] == R.WEAK).all()
    want = st.copy()
    want[path] = R.STRONG
    assert np.array_equal(out, want)
    # a device map in, a device map out; the caller's map is not written
    dev = torch.from_numpy(np.stack([st, st.T.copy()])).cuda()
    out = eng.canny_hysteresis(dev)
    assert out.is_cuda and np.array_equal(host(dev[0]), st)
    assert np.array_equal(host(out[0]), want) and np.array_equal(host(out[1]), want.T)
    # nothing strong: one batch of sweeps, nothing changes
    weak = np.where(st == R.STRONG, R.WEAK, st).astype(np.uint8)
    assert np.array_equal(eng.canny_hysteresis(weak[None])[0], weak)


def test_degenerate_inputs(eng):
    assert not eng.canny(np.full((2, 40, 70, 3), 93, np.uint8), 100, 200).any()
    rng = np.random.default_rng(5)
    for shape in ((2, 1, 75, 3), (2, 75, 1, 3), (1, 1, 1, 1), (2, 1, 130, 1), (1, 3, 2, 3)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        for lo, hi in ((100, 200), (0, 0)):
            assert np.array_equal(eng.canny(img, lo, hi), R.canny_batch(img, lo, hi)), (shape, lo, hi)


@pytest.mark.parametrize("mul,add", [(2.0, -1.0), (1.0, 0.0)])
@pytest.mark.parametrize("c_off", [0, 3])
def test_float_form(eng, c_off, mul, add):
    import torch
    for H, W_ in ((37, 53), (64, 64)):   # H * W odd, and a multiple of 4 (the vector stores)
        img, refs = blob_case(H, W_, 3)
        ref = refs[(100, 200)]
        hwc3 = np.stack([A.HWC3(r) for r in ref]).transpose(0, 3, 1, 2)
        want = (hwc3.astype(np.float32) / np.float32(255.0)) * np.float32(mul) + np.float32(add)
        out = torch.full((3, 6, H, W_), float(SENTINEL), dtype=torch.float32, device="cuda")
        edges = eng.canny(torch.from_numpy(img.copy()).cuda(), 100, 200, out=out, c_off=c_off, mul=mul, add=add)
        got = host(out)
        assert np.array_equal(host(edges), ref)
        assert np.array_equal(got[:, c_off:c_off + 3].view(np.uint32), want.view(np.uint32))
        rest = [c for c in range(6) if not c_off <= c < c_off + 3]
        assert (got[:, rest] == SENTINEL).all()
        # a host tensor: the same bits, the other channels left alone
        out_h = np.full((3, 6, H, W_), SENTINEL, np.float32)
        eng.canny(img, 100, 200, out=out_h, c_off=c_off, mul=mul, add=add)
        assert np.array_equal(out_h.view(np.uint32), got.view(np.uint32))


def test_memory_spaces_and_allocations(eng):
    import torch
    img, refs = blob_case(130, 67, 3)
    ref = refs[(100, 200)]
    dev = torch.from_numpy(img.copy()).cuda()
    got = eng.canny(dev, 100, 200)
    assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(host(got), ref)
    assert np.array_equal(eng.canny(img, 100, 200), ref)                       # NumPy in, NumPy out
    assert np.array_equal(eng.canny(dev, 100, 200, host=True), ref)            # device in, NumPy out
    cpu_t = eng.canny(torch.from_numpy(img.copy()), 100, 200)                         # CPU tensor in, device out
    assert cpu_t.is_cuda and np.array_equal(host(cpu_t), ref)
    out = torch.empty((3, 3, 130, 67), dtype=torch.float32, device="cuda")
    eng.canny(img, 100, 200, out=out)
    n = eng.stat("image_allocs")
    launches = eng.stat("launches")
    eng.canny(img, 100, 200)
    eng.canny(dev, 100, 200, out=out)
    eng.canny(img[:2, :100, :60], 100, 200)                                    # a smaller shape fits the same buffers
    assert eng.stat("image_allocs") == n
    assert eng.stat("launches") > launches and eng.stat("canny_sweeps") >= 1


def test_detector_surface(eng):
    import prompt_diffusion_amd
    assert prompt_diffusion_amd.CannyDetector is A.CannyDetector
    det = A.CannyDetector(eng)
    img, refs = blob_case(64, 64, 3)
    ref = eng.canny(img, 100, 200)
    assert np.array_equal(ref, refs[(100, 200)])
    one = det(img[1], 100, 200)
    assert isinstance(one, np.ndarray) and one.dtype == np.uint8 and np.array_equal(one, ref[1])
    grey, grey_refs = blob_case(64, 64, 1)
    assert np.array_equal(det(grey[0, :, :, 0], 100, 200), grey_refs[(100, 200)][0])   # HW
    assert np.array_equal(det(grey[0], 100, 200), grey_refs[(100, 200)][0])            # HW1
    h = det.detect(img, 100, 200, device=False)
    d = det.detect(img, 100, 200, device=True)
    assert isinstance(h, np.ndarray) and d.is_cuda
    assert np.array_equal(h, ref) and np.array_equal(host(d), ref)


def test_argument_errors_leave_the_engine_usable(eng):
    img, refs = blob_case(37, 53, 3)
    with pytest.raises(E.PdError, match="C 1 or 3"):
        eng.canny(np.zeros((1, 8, 8, 2), np.uint8), 100, 200)
    with pytest.raises(E.PdError, match="do not fit"):
        eng.canny(img, 100, 200, out=np.zeros((3, 5, 37, 53), np.float32), c_off=3)
    with pytest.raises(E.PdError, match="do not fit"):
        eng.canny(img, 100, 200, out=np.zeros((3, 6, 37, 53), np.float32), c_off=-1)
    with pytest.raises(E.PdError, match="finite"):
        eng.canny(img, float("nan"), 200)
    with pytest.raises(E.PdError, match="finite"):
        eng.canny(img, 100, float("inf"))
    a = E.pd_canny_args()
    a.src, a.B, a.H, a.W, a.C, a.mem_src = img.ctypes.data, 3, 37, 53, 3, E.PD_MEM_HOST
    a.low, a.high = 100.0, 200.0
    assert eng.lib.pd_canny(eng._h, C.byref(a)) != 0                           # no destination
    assert b"no destination" in eng.lib.pd_last_error()
    assert np.array_equal(eng.canny(img, 100, 200), refs[(100, 200)])
