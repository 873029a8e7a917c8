"""HED edge detector on the GPU (pd_hed_detect, Engine.hed, annotators.HEDdetector) against the reference Network's own outputs
(tests/golden/hed.npz, make_golden_hed.py) and, for the two element-wise kernels, against torch on the CPU.

Parity is `max |diff| / max |ref|` of each of the five side maps and of the edge map.  The bounds are the project's for a conv
stack (test_vae_encoder_gpu.py): f32 1e-4, f16x2 1e-4, f16 4e-3, bf16 3e-2.  Every map meets them in every mode (largest measured:
f32 2.7e-6, f16x2 7.1e-6, f16 2.3e-3 at 512x512, bf16 2.2e-2; DESIGN.md §7 lists all of them), so no map has a bound of its own."""
import dataclasses
import os

import numpy as np
import pytest

from prompt_diffusion_amd import annotators as A
from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import weights as W
from tests import hed_ref

pytestmark = pytest.mark.gpu

TOL = {"f32": 1e-4, "f16x2": 1e-4, "f16": 4e-3, "bf16": 3e-2}
PRECS = ["f32", "f16x2", "f16", "bf16"]
TINY_H = dataclasses.replace(W.TINY, hed=True)
SHAPES = {"tiny": (2, 3, 64, 64), "nonsq": (1, 3, 32, 48), "mid": (1, 3, 128, 128)}


def relerr(a, b):
    return float(np.abs(np.asarray(a) - b).max() / (np.abs(b).max() + 1e-30))


def images_from_key(key, shape):   # tests/golden/make_golden_hed.py
    return np.random.Generator(np.random.Philox(key=[79, int(key)])).uniform(0.0, 1.0, shape).astype(np.float32)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "hed.npz"))


@pytest.fixture(scope="module")
def sd():
    return W.synth_hed_state_dict()


def case_images(fx, tag):
    return fx[tag + "_images"] if tag + "_images" in fx else images_from_key(int(fx[tag + "_key"]), SHAPES[tag])


def _hed_engine(prec, sd, cfg=TINY_H):
    e = E.Engine(cfg, precision=prec)
    e.load_hed_state_dict(sd)
    assert e.hed_weights_missing() == 0
    return e


@pytest.fixture(scope="module")
def engines(sd):
    es = {p: _hed_engine(p, sd) for p in PRECS}
    yield es
    for e in es.values():
        e.close()


def check_parity(prec, tag, sides, edge, ref_sides, ref_edge):
    errs = [relerr(sides[:, i], ref_sides[:, i]) for i in range(5)] + [relerr(edge, ref_edge)]
    print(f"{tag} {prec}: side relerr " + " / ".join(f"{v:.3e}" for v in errs[:5]) + f", edge {errs[5]:.3e}")
    for i, v in enumerate(errs):
        assert v < TOL[prec], (prec, tag, i, v)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tag", ["tiny", "nonsq", "mid"])
def test_sides_and_edge_match_reference(fx, engines, tag, prec):
    e = engines[prec]
    assert e.weights_missing() > 0 and e.vae_weights_missing() > 0   # the detector needs none of the other networks
    x = case_images(fx, tag)
    sides, edge = e.hed(x, what="sides"), e.hed(x, what="edge")
    assert sides.shape == fx[tag + "_sides"].shape and edge.shape == fx[tag + "_edge"].shape
    check_parity(prec, tag, sides, edge, fx[tag + "_sides"], fx[tag + "_edge"])
    # the edge map is the combine + sigmoid of the engine's own side maps
    cw, cb = W.synth_hed_state_dict()["hed.netCombine.0.weight"].reshape(5), W.synth_hed_state_dict()["hed.netCombine.0.bias"]
    z = np.tensordot(cw, sides.astype(np.float64), axes=(0, 1)) + float(cb[0])      # [B, H, W]
    assert np.abs(edge[:, 0] - 1.0 / (1.0 + np.exp(-z))).max() <= 1e-6


def test_channel_order_is_rgb_in_bgr_inside(fx, engines):
    """The channel-reversed image is a different input: were the flip missing (or done twice) this is what the fixture would see."""
    rev = np.ascontiguousarray(fx["tiny_images"][:, ::-1])
    sides = engines["f32"].hed(rev, what="sides")
    errs = [relerr(sides[:, i], fx["tiny_sides"][:, i]) for i in range(5)]
    print("channel-reversed input: side relerr " + " / ".join(f"{v:.3e}" for v in errs))
    assert min(errs) > 10 * TOL["f32"]


def _round_to(x, prec):
    import torch
    t = torch.from_numpy(x)
    if prec == "f16":
        return t.half().float().numpy()
    if prec == "bf16":
        return t.bfloat16().float().numpy()
    return x


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B,Cc,H,Wd", [(2, 64, 6, 10), (1, 512, 2, 6), (1, 128, 16, 4)])
def test_op_stage_tail_matches_torch(engines, prec, B, Cc, H, Wd):
    """Score head + 2x2 max-pool from one read.  The input is rounded to the storage type first, so the pooled map must be exact
    and the score differs from torch's by fp32 summation order only: at most 4 sqrt(C) 2^-24 sum_c |x_c w_c| (both sums' random-walk
    rounding error, with a factor of two to spare)."""
    import torch
    import torch.nn.functional as F
    g = np.random.default_rng(1000 * Cc + H)
    x = _round_to(g.uniform(-1, 1, (B, Cc, H, Wd)).astype(np.float32), prec)
    w = (g.standard_normal((1, Cc, 1, 1)) / np.sqrt(Cc)).astype(np.float32)
    b = np.array([0.3], np.float32)
    tx = torch.from_numpy(x)
    ref_s = F.conv2d(tx, torch.from_numpy(w), torch.from_numpy(b))[:, 0].numpy()
    ref_p = F.max_pool2d(tx, kernel_size=2, stride=2).numpy()
    tol = 4.0 * np.sqrt(Cc) * 2.0 ** -24 * float(np.abs(x * w).sum(axis=1).max())
    e = engines[prec]
    score, pooled = e.op_hed_stage_tail(x, w, b)
    assert score.shape == (B, H, Wd) and pooled.shape == ref_p.shape
    err = float(np.abs(score - ref_s).max())
    print(f"stage tail {prec} C {Cc} {H}x{Wd}: score abs err {err:.3e} (bound {tol:.3e})")
    assert err <= tol
    np.testing.assert_array_equal(pooled, ref_p)
    score2, none = e.op_hed_stage_tail(x, w, b, pool=False)       # stage 5: the score only
    assert none is None
    np.testing.assert_array_equal(score2, score)


def test_op_stage_tail_odd_size_without_pool(engines):
    """Stage 5 of a 32x48 image is 2x3: quads hang over the right edge."""
    import torch
    import torch.nn.functional as F
    g = np.random.default_rng(9)
    x = g.uniform(-1, 1, (2, 512, 3, 5)).astype(np.float32)
    w = (g.standard_normal((1, 512, 1, 1)) / np.sqrt(512)).astype(np.float32)
    b = np.array([-0.1], np.float32)
    ref = F.conv2d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b))[:, 0].numpy()
    score, _ = engines["f32"].op_hed_stage_tail(x, w, b, pool=False)
    assert np.abs(score - ref).max() <= 4.0 * np.sqrt(512) * 2.0 ** -24 * float(np.abs(x * w).sum(axis=1).max())


@pytest.mark.parametrize("prec", ["f32", "f16"])
@pytest.mark.parametrize("B,H,Wd", [(2, 16, 16), (1, 48, 80), (1, 32, 48)])
def test_op_fuse_matches_torch(engines, prec, B, H, Wd):
    """Bilinear upsample (align_corners=False) x 2^i, combine, sigmoid: fp32 in every engine mode, <= 1e-6 absolute."""
    import torch
    import torch.nn.functional as F
    g = np.random.default_rng(H * 100 + Wd)
    maps = [g.standard_normal((B, 1, H >> i, Wd >> i)).astype(np.float32) for i in range(5)]
    cw = g.uniform(-0.6, 0.6, 5).astype(np.float32)
    cb = np.array([0.05], np.float32)
    ups = torch.cat([F.interpolate(torch.from_numpy(m), size=(H, Wd), mode="bilinear", align_corners=False) for m in maps], 1)
    ref_edge = torch.sigmoid(F.conv2d(ups, torch.from_numpy(cw).view(1, 5, 1, 1), torch.from_numpy(cb))).numpy()
    e = engines[prec]
    sides = e.op_hed_fuse(maps, cw, cb, what="sides")
    edge = e.op_hed_fuse(maps, cw, cb, what="edge")
    assert sides.shape == (B, 5, H, Wd) and edge.shape == (B, 1, H, Wd)
    es, ee = float(np.abs(sides - ups.numpy()).max()), float(np.abs(edge - ref_edge).max())
    print(f"fuse {prec} {H}x{Wd}: sides abs err {es:.3e}, edge abs err {ee:.3e}")
    assert es <= 1e-6 and ee <= 1e-6


def test_full_size_f16_dispatch(sd, capfd):
    """1 x 3 x 512 x 512 in f16, the shapes the demo runs, against the restatement in fp32 on the CPU."""
    x = images_from_key(4, (1, 3, 512, 512))
    ref_sides, ref_edge = hed_ref.detect_rgb(sd, x)
    e = _hed_engine("f16", sd)
    capfd.readouterr()
    e.set_option("verbose", 2)
    sides = e.hed(x, what="sides")
    e.set_option("verbose", 0)
    lines = [l for l in capfd.readouterr().err.splitlines() if l.startswith("[pdengine] gemm")]
    edge = e.hed(x, what="edge")
    e.close()
    print("\n".join(lines))
    assert len(lines) == 13 and all("taps 9 stride 1" in l and "act 5" in l for l in lines)
    # the layers that carry the bytes run on the LDS-patch kernels
    for rows, n in ((512 * 512, 64), (256 * 256, 128)):
        big = [l for l in lines if f"M {rows} N {n} K {9 * n} " in l]
        assert big and all("patch" in l for l in big), big
    check_parity("f16", "512x512", sides, edge, ref_sides, ref_edge)


def test_batch_of_eight_equals_batch_of_one(fx, engines):
    """Eight copies of one image give eight identical results, and the detector's output for them is that of the single image to
    <= 1e-6.  The side maps get a bound of their own: a batch of 8 and a batch of 1 take different kernels (the split-K counts
    and the patch / implicit-GEMM choice follow the number of rows), so the two are separate fp32 evaluations that differ in
    summation order.  With unit roundoff 2^-24, a random-walk error of 2^-24 sqrt(K) per layer at the longest reduction
    K = 4608, 13 layers adding in quadrature and two independent evaluations: 2^-24 sqrt(4608 * 13 * 2) = 2.1e-5 of the map's
    largest value.  Measured: 2.7e-7 / 3.9e-7 / 1.4e-6 / 8.0e-7 / 1.1e-6 (no normalisation layer damps it: the f32 parity errors
    against the reference are the same size)."""
    e = engines["f32"]
    x1 = fx["tiny_images"][:1]
    x8 = np.repeat(x1, 8, axis=0)
    one, eight = e.hed(x1, what="edge"), e.hed(x8, what="edge")
    np.testing.assert_array_equal(eight[1:], eight[:-1])
    err = float(np.abs(eight[:1] - one).max())
    print(f"B 8 against B 1: edge max abs diff {err:.3e}")
    assert err <= 1e-6
    one, eight = e.hed(x1, what="sides"), e.hed(x8, what="sides")
    np.testing.assert_array_equal(eight[1:], eight[:-1])
    errs = [relerr(eight[:1, c], one[:, c]) for c in range(5)]
    print("B 8 against B 1: side relerr " + " / ".join(f"{v:.3e}" for v in errs))
    assert max(errs) <= 2.0 ** -24 * np.sqrt(4608 * 13 * 2)


def test_device_tensors_are_bit_identical_to_host_arrays(fx, engines):
    import torch
    e = engines["f32"]
    for what in ("sides", "edge"):
        host = e.hed(fx["tiny_images"], what=what)
        dev = e.hed(torch.from_numpy(fx["tiny_images"]).cuda(), what=what)
        assert dev.is_cuda
        np.testing.assert_array_equal(dev.cpu().numpy(), host)


def _uint8_agrees(got, want, ref_edge):
    """Every pixel within one level, 99 % equal, and a differing pixel only where edge * 255 sits within the f32 parity bound of an
    integer (truncation turns that into a whole level)."""
    d = got.astype(np.int32) - want.astype(np.int32)
    assert np.abs(d).max() <= 1
    assert (d == 0).mean() >= 0.99
    v = ref_edge.astype(np.float32) * np.float32(255.0)
    near = np.abs(v - np.rint(v)) <= 255.0 * TOL["f32"]
    assert near[d != 0].all()


def test_detector_uint8(fx, sd, engines):
    e = engines["f32"]
    # the engine's float map through the detector's uint8 step against the fixture's
    edge = e.hed(fx["tiny_images"], what="edge")
    _uint8_agrees(A.edge_to_uint8(edge[:, 0]), hed_ref.to_uint8(fx["tiny_edge"][:, 0]), fx["tiny_edge"][:, 0])
    # HEDdetector end to end on uint8 images against the restatement of HEDdetector.__call__
    det = A.HEDdetector(e)
    imgs = np.rint(fx["tiny_images"].transpose(0, 2, 3, 1) * 255.0).astype(np.uint8)
    batch = det.detect(imgs)
    assert batch.dtype == np.uint8 and batch.shape == (2, 64, 64)
    for i in range(2):
        img = imgs[i]
        got = det(img)
        np.testing.assert_array_equal(got, batch[i])
        bgr = np.ascontiguousarray(img[:, :, ::-1].transpose(2, 0, 1))[None].astype(np.float32) / np.float32(255.0)
        import torch
        with torch.no_grad():
            _, ref_edge = hed_ref.forward_bgr(sd, torch.from_numpy(bgr))
        _uint8_agrees(got, hed_ref.detector(sd, img), ref_edge[0, 0].numpy())


def _sample_kw(B=1, h=8, w=8):
    inp = W.synth_inputs(W.TINY, B, h, w)
    return dict(x_T=inp["x_T"], ctx_cond=inp["ctx_cond"], ctx_uncond=inp["ctx_uncond"], pair=inp["pair"], query=inp["query"],
                steps=4, cfg_scale=7.5)


def test_default_engine_is_unchanged(fx, sd):
    """Registry, sampling, decode and encode of an engine are bit-identical whether or not it carries (and has run) the detector."""
    base = dataclasses.replace(W.TINY, vae_encoder=True)
    g = np.random.Generator(np.random.Philox(key=[5, 6]))
    z = g.standard_normal((2, 4, 8, 8), dtype=np.float32)
    img = np.ascontiguousarray(fx["tiny_images"] * 2.0 - 1.0)
    got = []
    for cfg in (base, dataclasses.replace(base, hed=True)):
        e = E.Engine(cfg, precision="f16")
        e.load_state_dict(W.synth_state_dict(cfg))
        for n, a in list(W.synth_vae_state_dict(cfg).items()) + list(W.synth_vae_encoder_state_dict(cfg).items()):
            e.load_tensor(n, a)
        if cfg.hed:
            assert e.hed_weights_missing() == 38
            e.load_hed_state_dict(sd)
            e.hed(fx["tiny_images"])
        else:
            assert e.hed_weights_missing() == 0
        assert e.weights_missing() == 0
        got.append((e.param_names(), e.ddim_sample(**_sample_kw()), e.vae_decode(z), e.vae_encode(img, mode="moments")))
        e.close()
    assert got[1][0] == got[0][0] + [(n, tuple(s)) for n, s, _ in W.hed_spec()]
    for a, b in zip(got[0][1:], got[1][1:]):
        np.testing.assert_array_equal(a, b)


def test_refused_inputs(fx, sd):
    x = fx["tiny_images"]
    plain = E.Engine(W.TINY, precision="f32")
    with pytest.raises(E.PdError, match="no HED edge detector"):
        plain.hed(x)
    assert plain.hed_weights_missing() == 0
    plain.close()
    e = E.Engine(TINY_H, precision="f32")
    assert e.hed_weights_missing() == 38
    with pytest.raises(E.PdError, match="'hed.netVggOne.0.weight'"):
        e.hed(x)
    first = "hed.netVggOne.0.weight"
    e.load_tensor(first, sd[first])
    with pytest.raises(E.PdError, match="'hed.netVggOne.0.bias'"):
        e.hed(x)
    e.load_hed_state_dict(sd)
    names = e.param_names()
    assert e.lib.pd_hed_configure(e._h) == 0 and e.param_names() == names and e.hed_weights_missing() == 0   # idempotent
    e.load_state_dict(W.synth_state_dict(W.TINY))
    e.sample_begin(**_sample_kw())
    with pytest.raises(E.PdError, match="end the sampling session first"):
        e.hed(x)
    e.sample_end()
    for shape in ((1, 3, 60, 64), (1, 3, 64, 72), (1, 3, 8, 64)):
        with pytest.raises(E.PdError, match="multiples of 16"):
            e.hed(np.zeros(shape, np.float32))
    with pytest.raises(ValueError):
        e.hed(x, what="maps")
    with pytest.raises(ValueError):
        e.hed(np.zeros((1, 4, 64, 64), np.float32))
    out = np.empty((2, 5, 64, 64), np.float32)
    assert e.lib.pd_hed_detect(e._h, x.ctypes.data, 2, 64, 64, E.PD_MEM_HOST, 7, out.ctypes.data) != 0
    assert "unknown `what`" in e.lib.pd_last_error().decode()
    # still usable
    sides = e.hed(x, what="sides")
    for i in range(5):
        assert relerr(sides[:, i], fx["tiny_sides"][:, i]) < TOL["f32"]
    e.close()
