"""The image ends on the GPU (pd_image_load / pd_image_store, Engine.image_load / image_store, the pipelines' device_images switch,
HEDdetector.detect(device=True)).  Everything is specified by integer or single-rounding fp32 arithmetic, so every comparison is
np.array_equal: against Pillow's Image.resize plus the NumPy value maps of tests/image_ref.py, and against the host paths of the
pipelines and the annotator."""
import dataclasses

import numpy as np
import pytest

from prompt_diffusion_amd import annotators as A
from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import weights as W
from prompt_diffusion_amd.pipeline import EngineGenerator, PromptDiffusionImg2ImgPipeline, PromptDiffusionPipeline
from prompt_diffusion_amd.schedulers import UniPCMultistepScheduler
from tests import image_ref as R

pytestmark = pytest.mark.gpu

CFG = dataclasses.replace(W.TINY, vae_encoder=True)
SHAPE_IDS = [f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in R.SHAPES]
SENTINEL = np.float32(-7.25)


def _engine(prec, cfg=CFG):
    e = E.Engine(cfg, precision=prec)
    e.load_state_dict({**W.synth_state_dict(cfg), **W.synth_vae_state_dict(cfg)})
    for n, a in W.synth_vae_encoder_state_dict(cfg).items():
        e.load_tensor(n, a)
    assert e.weights_missing() == 0 and e.vae_weights_missing() == 0 and e.vae_encoder_weights_missing() == 0
    return e


@pytest.fixture(scope="module")
def engines():
    es = {p: _engine(p) for p in ("f32", "f16")}
    yield es
    for e in es.values():
        e.close()


@pytest.fixture(scope="module")
def eng(engines):
    return engines["f32"]


_REF = {}


def reference(src, dst, filt, batch):
    """(uint8 pictures [batch, Hs, Ws, 3], Pillow's resize of them [batch, H, W, 3]); computed once per case"""
    key = (src, dst, filt, batch)
    if key not in _REF:
        img = R.seeded_image(src, seed=3, batch=batch)
        ref = R.pil_resize(img, dst, filt)
        img.setflags(write=False)
        ref.setflags(write=False)
        _REF[key] = (img, ref)
    return _REF[key]


def host(x):
    return x.cpu().numpy() if E._is_torch(x) else np.asarray(x)


# ------------------------------------------------------------------ image_load
@pytest.mark.parametrize("filt", ["lanczos", "box"])
@pytest.mark.parametrize("src,dst", R.SHAPES, ids=SHAPE_IDS)
def test_image_load_matches_pillow(eng, src, dst, filt):
    import torch
    img, ref = reference(src, dst, filt, 2)
    for mul, add in ((1.0, 0.0), (2.0, -1.0)):
        want = R.load_value(ref, mul, add)
        got = eng.image_load(img, dst, mul=mul, add=add, filter=filt)                       # host source, CUDA tensor out
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (2, 3) + tuple(dst)
        assert np.array_equal(host(got), want)
        dev = eng.image_load(torch.from_numpy(np.array(img)).cuda(), dst, mul=mul, add=add, filter=filt)   # device source
        assert np.array_equal(host(dev), want)
    back = eng.image_load(img, dst, filter=filt, host=True)                                 # host result
    assert isinstance(back, np.ndarray) and np.array_equal(back, R.load_value(ref, 1.0, 0.0))
    cpu_t = eng.image_load(torch.from_numpy(np.array(img)), dst, filter=filt)               # CPU torch source
    assert np.array_equal(host(cpu_t), R.load_value(ref, 1.0, 0.0))


@pytest.mark.parametrize("src,dst", R.SHAPES, ids=SHAPE_IDS)
def test_image_load_channel_offset_keeps_the_other_channels(eng, src, dst):
    import torch
    img, ref = reference(src, dst, "lanczos", 2)
    want = R.load_value(ref, 2.0, -1.0)
    out = torch.full((2, 6) + tuple(dst), float(SENTINEL), dtype=torch.float32, device="cuda")
    got = eng.image_load(img, dst, out=out, c_off=3, mul=2.0, add=-1.0)
    assert got is out
    o = host(out)
    assert np.array_equal(o[:, 3:], want)
    assert (o[:, :3] == SENTINEL).all()                                                     # the sentinel survives in channels 0 - 2
    eng.image_load(img, dst, out=out, c_off=0, mul=1.0, add=0.0)                            # the other half of a pair: no concat
    assert np.array_equal(host(out), np.concatenate([R.load_value(ref, 1.0, 0.0), want], axis=1))
    # a host destination keeps its other channels too
    hout = np.full((2, 6) + tuple(dst), SENTINEL, np.float32)
    eng.image_load(img, dst, out=hout, c_off=3, mul=2.0, add=-1.0)
    assert np.array_equal(hout[:, 3:], want) and (hout[:, :3] == SENTINEL).all()


@pytest.mark.parametrize("src,dst", R.SHAPES, ids=SHAPE_IDS)
def test_image_load_batch_modes(eng, src, dst):
    img, ref = reference(src, dst, "lanczos", 2)
    want = R.load_value(ref, 1.0, 0.0)
    one = eng.image_load(img[:1], dst, batch=3)                                             # Bs = 1 -> B = 3
    assert np.array_equal(host(one), np.repeat(want[:1], 3, axis=0))
    rep = eng.image_load(img, dst, batch=4, batch_mode="repeat")                            # Bs = 2 -> B = 4: np.repeat
    assert np.array_equal(host(rep), np.repeat(want, 2, axis=0))
    til = eng.image_load(img, dst, batch=4, batch_mode="tile")                              # ... and whole-batch repeats
    assert np.array_equal(host(til), np.tile(want, (2, 1, 1, 1)))
    assert not np.array_equal(host(rep), host(til))


def test_image_load_other_factors_round_twice(eng):
    """y = v * mul + add with the product and the sum each rounded once (no FMA), for factors where fusing would show."""
    img, ref = reference((37, 53), (64, 64), "lanczos", 2)
    fused = 0
    for mul, add in ((0.7, 0.1), (1.0 / 3.0, -0.3), (255.0, -127.5)):
        want = R.load_value(ref, mul, add)
        assert np.array_equal(host(eng.image_load(img, (64, 64), mul=mul, add=add)), want)
        v32 = (ref.astype(np.float32) / np.float32(255.0)).astype(np.float64)
        fma = (v32 * np.float64(np.float32(mul)) + np.float64(np.float32(add))).astype(np.float32).transpose(0, 3, 1, 2)
        fused += int((fma != want).sum())
    assert fused > 0          # the check can tell the two apart on these inputs


def test_image_load_allocates_once_and_refuses(eng):
    img, _ = reference((100, 80), (64, 128), "lanczos", 2)
    eng.image_load(img, (64, 128))
    n = eng.stat("image_allocs")
    assert n > 0
    for _ in range(3):
        eng.image_load(img, (64, 128))
        eng.image_load(img, (64, 128), mul=2.0, add=-1.0, batch=4)
    assert eng.stat("image_allocs") == n                                                    # same shapes: nothing allocated
    big = np.zeros((1, 64 * E.PD_RESAMPLE_MAX_SCALE + 1, 16, 3), np.uint8)
    with pytest.raises(E.PdError, match="PD_RESAMPLE_MAX_SCALE"):
        eng.image_load(big, (64, 16))
    with pytest.raises(E.PdError, match="divide"):
        eng.image_load(img, (64, 128), batch=3)
    with pytest.raises(E.PdError, match="do not fit"):
        eng.image_load(img, (64, 128), c_off=1)
    assert np.array_equal(host(eng.image_load(img, (64, 128))), R.load_value(R.pil_resize(img, (64, 128)), 1, 0))   # still works


# ------------------------------------------------------------------ image_store
def _tie_points(C, shape):
    """the 256 points 2 ((k + 0.5) / 255) - 1: x / 2 + 0.5 lands on (or one ulp beside) the rounding ties k + 0.5 of u * 255"""
    k = np.arange(256, dtype=np.float64)
    pts = (2.0 * ((k + 0.5) / 255.0) - 1.0).astype(np.float32)
    n = int(np.prod(shape))
    return np.resize(pts, C * n).reshape((shape[0], C) + tuple(shape[1:]))


@pytest.mark.parametrize("rounding", ["nearest_even", "trunc"])
@pytest.mark.parametrize("shape", [(1, 5, 7), (2, 64, 48)], ids=["1x5x7", "2x64x48"])
@pytest.mark.parametrize("C", [1, 3])
def test_image_store_matches_numpy(eng, C, shape, rounding):
    import torch
    B, H, Wd = shape
    x = np.random.default_rng([C, H]).uniform(-1.3, 1.3, (B, C, H, Wd)).astype(np.float32)
    ties = _tie_points(C, shape)
    full = _tie_points(C, (1, 16, 16))                      # all 256 of them in every channel, whatever `shape` holds
    unit = np.ascontiguousarray(np.linspace(-0.1, 1.1, B * C * H * Wd, dtype=np.float32).reshape(B, C, H, Wd))
    for arr, (mul, add) in ((x, (0.5, 0.5)), (ties, (0.5, 0.5)), (full, (0.5, 0.5)), (unit, (1.0, 0.0)), (x, (1.0, 0.0)),
                            (full, (0.37, 0.21))):
        want = R.store_value(arr, mul, add, rounding)
        got = eng.image_store(arr, mul=mul, add=add, rounding=rounding)                     # host source, CUDA tensor out
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want.shape == (arr.shape[0],) + arr.shape[2:] + (C,)
        assert np.array_equal(host(got), want)
        dev = eng.image_store(torch.from_numpy(arr).cuda(), mul=mul, add=add, rounding=rounding, host=True)   # device source, host out
        assert isinstance(dev, np.ndarray) and np.array_equal(dev, want)
    # the tie points really are ties for half-to-even against truncation: the two roundings differ there
    assert not np.array_equal(R.store_value(full, 0.5, 0.5, "nearest_even"), R.store_value(full, 0.5, 0.5, "trunc"))


def test_image_store_refuses(eng):
    with pytest.raises(ValueError, match="1 or 3"):
        eng.image_store(np.zeros((1, 2, 4, 4), np.float32))
    with pytest.raises(KeyError):
        eng.image_store(np.zeros((1, 3, 4, 4), np.float32), rounding="up")


# ------------------------------------------------------------------ pipelines: switch on == switch off
def _pil(hw, seed, n=None):
    from PIL import Image
    a = np.random.default_rng([seed, hw[0]]).integers(0, 256, ((n or 1),) + tuple(hw) + (3,), dtype=np.uint8)
    ims = [Image.fromarray(x, "RGB") for x in a]
    return ims if n else ims[0]


def _kw(src_hw, B=2):
    inp = W.synth_inputs(CFG, B, 16, 16, seed=29, unit_range=True)
    return dict(prompt_embeds=inp["ctx_cond"], negative_prompt_embeds=inp["ctx_uncond"], image=_pil(src_hw, 1),
                image_pair=[_pil(src_hw, 2, n=B), _pil(src_hw, 3)], height=128, width=128, num_inference_steps=5,
                guidance_scale=4.0, latents=inp["x_T"], control_guidance_end=0.8)


def _both(make_pipe, kw, **over):
    """(latents off, latents on, pil bytes off, pil bytes on): the same call with the switch off and on"""
    out = []
    for output_type in ("latent", "pil"):
        for on in (False, True):
            pipe = make_pipe()
            assert pipe._device_images is False                     # off by default
            if on:
                pipe.enable_device_images()
            fresh = {k: (v() if callable(v) else v) for k, v in over.items()}
            res = pipe(**dict(kw, output_type=output_type, **fresh)).images
            out.append(np.asarray(res) if output_type == "latent" else np.stack([np.asarray(im) for im in res]))
    return out


def _check(lat_off, lat_on, pil_off, pil_on, B=2):
    assert isinstance(lat_on, np.ndarray) and lat_on.dtype == np.float32 and lat_on.shape == (B, 4, 16, 16)
    assert np.isfinite(lat_off).all() and np.array_equal(lat_on, lat_off)
    assert pil_on.dtype == np.uint8 and pil_on.shape == (B, 128, 128, 3)
    assert np.array_equal(pil_on, pil_off)
    assert len(np.unique(pil_off)) > 4                              # a picture, not a constant


SIZES = [(100, 90), (128, 128)]
SIZE_IDS = ["resized", "native"]


@pytest.mark.parametrize("src_hw", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_pipeline_ddim(engines, prec, src_hw):
    e = engines[prec]
    launches = e.stat("launches")
    _check(*_both(lambda: PromptDiffusionPipeline(e), _kw(src_hw)))
    assert e.stat("launches") > launches
    # the constructor argument and disable_device_images()
    pipe = PromptDiffusionPipeline(e, device_images=True)
    assert pipe._device_images is True
    pipe.disable_device_images()
    assert pipe._device_images is False


@pytest.mark.parametrize("src_hw", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_pipeline_fused_unipc(engines, prec, src_hw):
    e = engines[prec]
    _check(*_both(lambda: PromptDiffusionPipeline(e, scheduler=UniPCMultistepScheduler(), fuse_scheduler=True), _kw(src_hw)))


@pytest.mark.parametrize("src_hw", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_pipeline_img2img_pil_init_image(engines, prec, src_hw):
    e = engines[prec]
    kw = _kw(src_hw)
    kw["control_image"] = kw.pop("image")
    kw.pop("latents")
    kw.update(image=_pil(src_hw, 4), strength=0.6, num_inference_steps=10)
    _check(*_both(lambda: PromptDiffusionImg2ImgPipeline(e), kw, generator=lambda: EngineGenerator(1234)))


@pytest.mark.parametrize("src_hw", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_pipeline_callback_takes_the_per_step_driver(engines, prec, src_hw):
    e = engines[prec]
    seen = []
    res = _both(lambda: PromptDiffusionPipeline(e), _kw(src_hw),
                callback_on_step_end=lambda: (lambda p, i, t, k: seen.append(np.array(k["latents"])) or {}))
    _check(*res)
    assert len(seen) == 4 * 5
    for i in range(5):
        assert np.array_equal(seen[i], seen[5 + i])                 # the per-step latents agree as well
    assert np.array_equal(res[0], _both(lambda: PromptDiffusionPipeline(e), _kw(src_hw))[1])     # and equal the fused loop's


def test_pipeline_falls_back_per_input(eng):
    """Inputs that are not the device path's kind keep the host code, one by one: a float array, an 'L' image, a reduction beyond
    the bound; the results still equal the switch-off call."""
    from PIL import Image
    kw = _kw((100, 90))
    kw["image"] = np.asarray(kw["image"].resize((128, 128), resample=Image.LANCZOS), dtype=np.float32)[None] / 255.0
    kw["image_pair"][1] = kw["image_pair"][1].convert("L")
    tall = np.random.default_rng(5).integers(0, 256, (128 * E.PD_RESAMPLE_MAX_SCALE + 8, 100, 3), dtype=np.uint8)
    kw["image_pair"][0] = Image.fromarray(tall, "RGB")
    _check(*_both(lambda: PromptDiffusionPipeline(eng), kw))


# ------------------------------------------------------------------ annotator
@pytest.mark.parametrize("shape", [(2, 64, 64, 3), (1, 32, 48, 3)], ids=["2x64x64", "1x32x48"])
def test_hed_detect_on_the_device(shape):
    cfg = dataclasses.replace(W.TINY, hed=True)
    e = E.Engine(cfg, precision="f32")
    try:
        e.load_hed_state_dict(W.synth_hed_state_dict())
        det = A.HEDdetector(e)
        x = np.random.default_rng(shape[1]).integers(0, 256, shape, dtype=np.uint8)
        off, on = det.detect(x), det.detect(x, device=True)
        assert on.dtype == np.uint8 and on.shape == shape[:3]
        assert np.array_equal(on, off)
        assert len(np.unique(off)) > 4
    finally:
        e.close()
