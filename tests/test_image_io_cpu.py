"""pd_resample_coefficients on the host (no GPU): Pillow's 8-bit resampling tables.  The tables, evaluated by the integer two-pass
of tests/image_ref.py, must reproduce PIL.Image.resize byte for byte; three cases are also pinned as data in
tests/golden/image_io.npz (make_golden_image_io.py), tables included, whatever Pillow is installed."""
import ctypes as C
import os

import numpy as np
import pytest

from prompt_diffusion_amd import engine as E
from tests import image_ref as R
from tests.golden.make_golden_image_io import CASES

FILTERS = ("lanczos", "box")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(E.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return E.load_library()


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "image_io.npz"))


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("src,dst", R.SHAPES, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in R.SHAPES])
def test_tables_reproduce_pillow(lib, src, dst, filt):
    for seed in (0, 1):
        img = R.seeded_image(src, seed)
        got = R.resize_u8(img, dst, E.resample_coefficients, filt)
        ref = R.pil_resize(img, dst, filt)
        assert got.shape == ref.shape == tuple(dst) + (3,)
        assert np.array_equal(got, ref), f"{int((got != ref).sum())} differing bytes"
        if src == dst:
            assert np.array_equal(got, img)        # both passes skipped


def test_checkerboard_needs_the_clip(lib):
    """The case is there for the clip: without it the Lanczos sums leave [0, 255] on the checkerboard."""
    src, dst = R.CHECKER
    img = R.seeded_image(src, 0).astype(np.int64)
    bounds, kk = E.resample_coefficients(src[1], dst[1], "lanczos")
    acc = np.stack([(img[:, x0:x0 + n] * kk[i, :n, None].astype(np.int64)).sum(1) for i, (x0, n) in enumerate(bounds)], 1)
    v = (acc + (1 << 21)) >> 22
    assert v.min() < 0 or v.max() > 255
    assert np.abs(acc).max() + (1 << 21) < 2 ** 31      # and the int32 accumulator of the kernels holds them


@pytest.mark.parametrize("tag,src,dst,filt", CASES, ids=[c[0] for c in CASES])
def test_golden_tables_and_pixels(lib, fx, tag, src, dst, filt):
    img, ref = fx[f"{tag}_in"], fx[f"{tag}_out"]
    assert img.shape == tuple(src) + (3,) and ref.shape == tuple(dst) + (3,)
    assert np.array_equal(img, R.seeded_image(src, seed=11))
    for axis, (i, o) in (("h", (src[1], dst[1])), ("v", (src[0], dst[0]))):
        bounds, kk = E.resample_coefficients(i, o, filt)
        assert np.array_equal(bounds, fx[f"{tag}_bounds_{axis}"])
        assert np.array_equal(kk, fx[f"{tag}_kk_{axis}"])
    stored = {(src[1], dst[1]): (fx[f"{tag}_bounds_h"], fx[f"{tag}_kk_h"]), (src[0], dst[0]): (fx[f"{tag}_bounds_v"], fx[f"{tag}_kk_v"])}
    assert np.array_equal(R.resize_u8(img, dst, lambda i, o, f: stored[(i, o)], filt), ref)     # the pinned pixels from the pinned tables
    assert np.array_equal(R.pil_resize(img, dst, filt), ref)                                    # and the installed Pillow agrees


@pytest.mark.parametrize("filt", FILTERS)
def test_size_query_padding_and_bounds(lib, filt):
    S = 3.0 if filt == "lanczos" else 0.5
    code = E.RESAMPLE_FILTERS[filt]
    assert (E.PD_RESAMPLE_LANCZOS, E.PD_RESAMPLE_BOX) == (1, 4) == (R.PIL_FILTER["lanczos"], R.PIL_FILTER["box"])
    for i, o in ((53, 64), (64, 37), (300, 192), (511, 64), (16, 128), (64, 64), (1, 5), (8, 1)):
        ks = C.c_int32(-1)
        assert lib.pd_resample_coefficients(i, o, code, C.byref(ks), None, None) == 0      # the size query writes ksize only
        want = 2 * int(np.ceil(S * max(i / o, 1.0))) + 1
        assert ks.value == want == E.resample_ksize(i, o, filt)
        bounds, kk = E.resample_coefficients(i, o, filt)
        assert bounds.shape == (o, 2) and kk.shape == (o, want) and bounds.dtype == kk.dtype == np.int32
        xmin, cnt = bounds[:, 0], bounds[:, 1]
        assert (xmin >= 0).all() and (cnt >= 1).all() and (cnt <= want).all() and (xmin + cnt <= i).all()   # never past the source
        assert (np.diff(xmin) >= 0).all()
        for x in range(o):
            assert not kk[x, cnt[x]:].any()                                                # zero padded
        assert (np.abs(kk.sum(1) - (1 << 22)) <= want).all()                               # normalised weights, rounded per tap


def test_refusals(lib):
    ks = C.c_int32(-1)
    lan = E.PD_RESAMPLE_LANCZOS
    assert E.PD_RESAMPLE_MAX_SCALE >= 8
    m = E.PD_RESAMPLE_MAX_SCALE
    assert lib.pd_resample_coefficients(64 * m, 64, lan, C.byref(ks), None, None) == 0     # exactly the bound passes
    for args, msg in (((64 * m + 1, 64, lan), b"PD_RESAMPLE_MAX_SCALE"), ((64, 64, 3), b"unknown filter"), ((0, 64, lan), b">= 1"),
                      ((64, 0, lan), b">= 1")):
        ks.value = -1
        assert lib.pd_resample_coefficients(*args, C.byref(ks), None, None) != 0
        assert msg in lib.pd_last_error(), lib.pd_last_error()
        assert ks.value == -1                                                              # nothing written
    with pytest.raises(E.PdError, match="PD_RESAMPLE_MAX_SCALE"):
        E.resample_coefficients(64 * m + 1, 64)
    assert not E.resample_supported((64 * m + 1, 64), (64, 64)) and E.resample_supported((64 * m, 3), (64, 300))
    b = np.zeros((4, 2), np.int32)
    assert lib.pd_resample_coefficients(8, 4, lan, C.byref(ks), b.ctypes.data, None) != 0  # bounds without kk


def test_value_maps_are_the_host_code():
    """The NumPy expressions the GPU tests compare against are the host code the image ends replace."""
    u8 = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1).repeat(3, 3)
    a = np.asarray(u8[0], dtype=np.float32) / 255.0                                       # prepare_image
    assert np.array_equal(R.load_value(u8, 1, 0)[0], a.transpose(2, 0, 1))
    assert np.array_equal(R.load_value(u8, 2, -1)[0], (a.transpose(2, 0, 1)[None] * np.float32(2.0) - np.float32(1.0))[0])   # _init_latents
    x = np.random.default_rng(0).uniform(-1.3, 1.3, (2, 3, 5, 7)).astype(np.float32)
    img = np.clip(x / 2 + 0.5, 0, 1).transpose(0, 2, 3, 1)                                # the pipeline's post-processing
    assert np.array_equal(R.store_value(x, 0.5, 0.5, "nearest_even"), (img * 255).round().astype("uint8"))
    from prompt_diffusion_amd.annotators import edge_to_uint8
    assert np.array_equal(R.store_value(x[:, :1], 1, 0, "trunc")[..., 0], edge_to_uint8(x[:, 0]))
