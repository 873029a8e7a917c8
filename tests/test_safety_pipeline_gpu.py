"""The safety checker inside PromptDiffusionPipeline on the tiny network: without a checker a call is what it was (same latents, same
images, same launches); with the engine's checker, thresholds of -1 flag every image (black pictures) and +1 none (untouched
pictures), with the image ends on the device and on the host; a callable checker and pictures the device preprocessing refuses are
still checked when the image ends are on the device."""
import dataclasses

import numpy as np
import pytest

from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import weights as W
from prompt_diffusion_amd.pipeline import PromptDiffusionPipeline
from tests import clip_vision_ref as R

pytestmark = pytest.mark.gpu
TOWER = R.CONFIGS["A"][0]
B, HW, STEPS = 2, 64, 2


@pytest.fixture(scope="module")
def eng():
    cfg = dataclasses.replace(W.TINY, clip_vision=(TOWER,), safety_checker=True)
    e = E.Engine(cfg, precision="f32")
    e.load_state_dict({**W.synth_state_dict(W.TINY), **W.synth_vae_state_dict(W.TINY)}, strict=False)
    e.load_clip_vision_state_dict({**R.synth_state_dict(TOWER), **{"safety_checker." + k: v for k, v in R.synth_safety().items() if k != "embeds"}},
                                  TOWER.prefix)
    assert e.weights_missing() == 0 and e.vae_weights_missing() == 0 and e.safety_weights_missing() == 0
    yield e
    e.close()


def _kw():
    inp = W.synth_inputs(W.TINY, B, HW // 8, HW // 8, seed=5, unit_range=True)
    a, b = inp["pair"][:, :3], inp["pair"][:, 3:]
    return dict(prompt_embeds=inp["ctx_cond"], negative_prompt_embeds=inp["ctx_uncond"], image=inp["query"].transpose(0, 2, 3, 1),
                image_pair=[a.transpose(0, 2, 3, 1), b.transpose(0, 2, 3, 1)], num_inference_steps=STEPS, guidance_scale=3.0,
                latents=inp["x_T"])


def _thresholds(e, value):
    s = R.with_thresholds(R.synth_safety(), value)
    for k in ("concept_embeds_weights", "special_care_embeds_weights"):
        e.load_tensor("safety_checker." + k, s[k])


@pytest.mark.parametrize("device_images", [False, True])
def test_no_checker_is_the_old_call(eng, device_images):
    """the switch absent against safety_checker=None: same latents, same pictures, same number of launches, nsfw None"""
    kw = _kw()
    runs = []
    for pipe in (PromptDiffusionPipeline(eng, device_images=device_images),
                 PromptDiffusionPipeline(eng, device_images=device_images, safety_checker=None, feature_extractor=None, image_encoder=None,
                                         requires_safety_checker=False)):
        n0 = eng.stat("launches")
        lat = pipe(output_type="latent", **kw)
        n1 = eng.stat("launches")
        out = pipe(output_type="pil", **kw)
        runs.append((np.asarray(lat.images), [np.asarray(im) for im in out.images], n1 - n0, eng.stat("launches") - n1))
        assert lat.nsfw_content_detected is None and out.nsfw_content_detected is None
        assert pipe(output_type="pil", return_dict=False, **kw)[1] is None
    assert np.array_equal(runs[0][0], runs[1][0]) and all(np.array_equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    assert runs[0][2:] == runs[1][2:]


@pytest.mark.parametrize("device_images", [False, True])
def test_checker_flags_all_or_none(eng, device_images):
    kw = _kw()
    plain = PromptDiffusionPipeline(eng, device_images=device_images)
    base = [np.asarray(im) for im in plain(output_type="pil", **kw).images]
    n_plain = eng.stat("launches")
    plain(output_type="pil", **kw)
    n_plain = eng.stat("launches") - n_plain
    pipe = PromptDiffusionPipeline(eng, device_images=device_images, safety_checker=True, requires_safety_checker=True)
    _thresholds(eng, 1.0)        # nothing can reach a threshold of +1
    n0 = eng.stat("launches")
    out = pipe(output_type="pil", **kw)
    assert eng.stat("launches") - n0 > n_plain                    # the tower did run
    assert out.nsfw_content_detected == [False] * B
    assert all(np.array_equal(np.asarray(im), b) for im, b in zip(out.images, base)) and any(b.any() for b in base)
    _thresholds(eng, -1.0)       # every cosine exceeds -1
    out = pipe(output_type="pil", **kw)
    assert out.nsfw_content_detected == [True] * B and len(out.images) == B
    assert all(np.asarray(im).shape == (HW, HW, 3) and not np.asarray(im).any() for im in out.images)
    img, flags = pipe(output_type="np", return_dict=False, **kw)
    assert flags == [True] * B and img.shape == (B, HW, HW, 3) and not img.any()
    lat = pipe(output_type="latent", **kw)
    assert lat.nsfw_content_detected is None and np.asarray(lat.images).any()     # latents are never checked
    # the reference's method on a decoded tensor in [-1, 1]
    x = np.random.default_rng(0).uniform(-1, 1, (B, 3, HW, HW)).astype(np.float32)
    y, f = pipe.run_safety_checker(x)
    assert f == [True] * B and not y.any() and x.any()
    _thresholds(eng, 1.0)
    y, f = pipe.run_safety_checker(x)
    assert f == [False] * B and y is x


class _FeatureExtractor:
    """stands in for CLIPImageProcessor on the host: any callable PIL pictures -> .pixel_values [B, 3, S, S] will do"""

    def __init__(self):
        self.seen = []

    def __call__(self, pics, return_tensors=None):
        self.seen.append((len(pics), pics[0].size, return_tensors))
        S = TOWER.image_size
        pv = np.stack([np.asarray(p.convert("RGB").resize((S, S)), np.float32).transpose(2, 0, 1) / 255 for p in pics])
        return type("Features", (), {"pixel_values": (pv - 0.5) / 0.25})()


def test_callable_checker_keeps_precedence_with_device_images(eng):
    """a checker the device branch of the image ends cannot run is still run: the call takes the host branch"""
    kw = _kw()
    base = [np.asarray(im) for im in PromptDiffusionPipeline(eng, device_images=True)(output_type="pil", **kw).images]
    seen = []

    def checker(images, clip_input):
        seen.append((tuple(images.shape), tuple(clip_input.shape)))
        return images, [True] + [False] * (len(images) - 1)         # diffusers' returns the images zeroed; this one leaves that to the caller

    _thresholds(eng, 1.0)       # the engine's own checker would flag nothing: the flags below are the callable's
    fe = _FeatureExtractor()
    n0 = eng.stat("launches")
    pipe = PromptDiffusionPipeline(eng, device_images=True, safety_checker=checker, feature_extractor=fe, requires_safety_checker=True)
    out = pipe(output_type="pil", **kw)
    assert out.nsfw_content_detected == [True, False] and seen == [((B, HW, HW, 3), (B, 3, TOWER.image_size, TOWER.image_size))]
    assert fe.seen == [(B, (HW, HW), "np")]
    assert not np.asarray(out.images[0]).any() and np.array_equal(np.asarray(out.images[1]), base[1]) and base[0].any()
    assert eng.stat("launches") > n0


def test_unsupported_reduction_is_still_checked_with_device_images(eng):
    """512 x 512 pictures into the 56-pixel tower are a 9.1 x reduction, beyond PD_RESAMPLE_MAX_SCALE: the engine's checker then reads the
    caller's feature_extractor output -- and without one the call fails instead of returning unchecked pictures"""
    big = 512
    assert not E.clip_preprocess_supported(big, big, TOWER.image_size)
    inp = W.synth_inputs(W.TINY, 1, big // 8, big // 8, seed=6, unit_range=True)
    a, b = inp["pair"][:, :3], inp["pair"][:, 3:]
    kw = dict(prompt_embeds=inp["ctx_cond"], negative_prompt_embeds=inp["ctx_uncond"], image=inp["query"].transpose(0, 2, 3, 1),
              image_pair=[a.transpose(0, 2, 3, 1), b.transpose(0, 2, 3, 1)], num_inference_steps=1, guidance_scale=3.0, latents=inp["x_T"])
    fe = _FeatureExtractor()
    pipe = PromptDiffusionPipeline(eng, device_images=True, safety_checker=True, feature_extractor=fe)
    _thresholds(eng, -1.0)
    out = pipe(output_type="pil", **kw)
    assert out.nsfw_content_detected == [True] and out.images[0].size == (big, big) and not np.asarray(out.images[0]).any()
    assert fe.seen == [(1, (big, big), "np")]
    _thresholds(eng, 1.0)
    out = pipe(output_type="pil", **kw)
    assert out.nsfw_content_detected == [False] and np.asarray(out.images[0]).any()
    with pytest.raises(ValueError, match="feature_extractor"):
        PromptDiffusionPipeline(eng, device_images=True, safety_checker=True)(output_type="pil", **kw)
