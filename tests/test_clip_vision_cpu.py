"""CPU-side checks of the CLIP image tower: Pillow's bicubic tables (pd_resample_coefficients_ex) against PIL byte for byte, the
NumPy restatements of tests/clip_vision_ref.py against tests/golden/clip_vision.npz (made by transformers and PIL themselves:
tests/golden/make_golden_clip_vision.py) and, where transformers is importable, against the live modules; the ctypes mirrors; and the
pipeline's run_safety_checker / encode_image surface against a stub engine.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import weights as W
from prompt_diffusion_amd.pipeline import PromptDiffusionPipeline
from tests import clip_vision_ref as R
from tests import image_ref

MEAN, STD = W.OPENAI_CLIP_MEAN, W.OPENAI_CLIP_STD


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "clip_vision.npz"))


# ------------------------------------------------------------------------------------------------ tables and preprocessing
def _pil_bicubic(img, hw):
    from PIL import Image
    return np.asarray(Image.fromarray(img, "RGB").resize((hw[1], hw[0]), resample=Image.BICUBIC))


@pytest.mark.parametrize("hw", R.PREP_SHAPES)
def test_bicubic_tables_reproduce_pil(hw, gold):
    """Image.resize(..., BICUBIC) byte for byte from the new tables, and the fixture's rows of it and of the processor's pixel_values"""
    H, W_ = hw
    img = R.synth_pictures(hw)
    k = f"prep_{H}x{W_}"
    assert R.crc(img[0]) == int(gold[k + "_img_crc"])
    Hr, Wr, top, left = R.resize_geometry(H, W_, 224)
    assert (Hr, Wr, top, left) == tuple(gold[k + "_geometry"]) == E.clip_preprocess_geometry(H, W_, 224)
    full, crop, pv = R.preprocess(img, 224, E.resample_coefficients_ex, MEAN, STD)
    assert (full[0] != _pil_bicubic(img[0], (Hr, Wr))).sum() == 0
    assert (crop[0][R.PREP_ROWS] != gold[k + "_bytes_rows"]).sum() == 0 and R.crc(crop[0]) == int(gold[k + "_bytes_crc"])
    assert R.ulp_diff(pv[0][:, R.PREP_ROWS], gold[k + "_pixel_values_rows"]) <= 1
    if int(gold[k + "_pixel_values_exact"]):
        assert R.crc(pv) == int(gold[k + "_pixel_values_crc"])


def test_bicubic_enlargement_and_old_entry():
    (H, W_), dst = R.ENLARGE
    img = R.synth_pictures((H, W_))[0]
    assert (image_ref.resize_u8(img, dst, E.resample_coefficients_ex, "bicubic") != _pil_bicubic(img, dst)).sum() == 0
    # the two older filters: the same tables from both entries; the older entry keeps refusing 3
    for f in ("lanczos", "box"):
        for a, b in zip(E.resample_coefficients(100, 37, f), E.resample_coefficients_ex(100, 37, f)):
            assert np.array_equal(a, b)
    ks = C.c_int32()
    lib = E.load_library()
    assert lib.pd_resample_coefficients(64, 64, 3, C.byref(ks), None, None) != 0 and b"unknown filter" in lib.pd_last_error()
    assert lib.pd_resample_coefficients_ex(64, 64, 2, C.byref(ks), None, None) != 0 and b"unknown filter" in lib.pd_last_error()
    assert lib.pd_resample_coefficients_ex(224 * 9, 224, 3, C.byref(ks), None, None) != 0 and b"PD_RESAMPLE_MAX_SCALE" in lib.pd_last_error()
    assert not E.clip_preprocess_supported(2048, 2048, 224) and E.clip_preprocess_supported(512, 512, 224)
    assert E.PD_RESAMPLE_BICUBIC == 3 and lib.pd_abi_version() == 2 and E.clip_patch_width(14) == 592


def test_processor_live():
    """the restatement against the installed CLIPImageProcessor itself"""
    tr = pytest.importorskip("transformers")
    from PIL import Image
    proc = tr.CLIPImageProcessor()
    for hw in R.PREP_SHAPES[:3]:
        img = R.synth_pictures(hw, seed=R.SEED + 1)
        ref = np.asarray(proc(Image.fromarray(img[0], "RGB"), return_tensors="np").pixel_values, np.float32)
        _, _, pv = R.preprocess(img, 224, E.resample_coefficients_ex, MEAN, STD)
        assert R.ulp_diff(pv, ref) <= 1
    # every byte value in every channel
    ramp = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (224, 256, 3))[:, :224].copy()
    ramp[:32, :32] = np.arange(224, 256, dtype=np.uint8)[None, :, None]
    ref = np.asarray(proc(Image.fromarray(ramp, "RGB"), return_tensors="np").pixel_values, np.float32)
    assert R.ulp_diff(R.normalize(ramp[None], MEAN, STD), ref) <= 1


# ------------------------------------------------------------------------------------------------ the tower
@pytest.mark.parametrize("name", sorted(R.CONFIGS))
def test_restatement_meets_fixture(name, gold):
    cfg, B = R.CONFIGS[name]
    sd, pv = R.synth_state_dict(cfg), R.synth_pixel_values(name)
    assert R.crc(pv) == int(gold[f"{name}_pv_crc"]) and R.crc(np.concatenate([v.ravel() for v in sd.values()])) == int(gold[f"{name}_sd_crc"])
    r = R.forward(sd, cfg, pv)
    assert R.relerr(r["image_embeds"], gold[f"{name}_image_embeds"]) < 1e-12
    assert R.relerr(r["pooler_output"], gold[f"{name}_pooler_output"]) < 1e-12
    assert R.relerr(r["hidden_states"][-2][:, R.HIDDEN_ROWS[name]], gold[f"{name}_hidden"]) < 1e-12
    # registry names = the shapes table, in order; the checkpoint spelling included
    names = list(W.clip_vision_param_shapes(cfg))
    assert names == list(sd) and any("pre_layrnorm" in n for n in names)
    assert names[-1] == ("safety_checker." if name == "A" else "image_encoder.") + "visual_projection.weight"


def test_restatement_live():
    tr = pytest.importorskip("transformers")
    torch = pytest.importorskip("torch")
    cfg, _ = R.CONFIGS["C"]
    sd, pv = R.synth_state_dict(cfg), R.synth_pixel_values("C")
    hc = tr.CLIPVisionConfig(hidden_size=cfg.hidden, intermediate_size=cfg.ff, projection_dim=cfg.proj_dim, num_hidden_layers=cfg.layers,
                             num_attention_heads=cfg.heads, image_size=cfg.image_size, patch_size=cfg.patch, hidden_act=cfg.act,
                             layer_norm_eps=cfg.eps, attn_implementation="sdpa")
    m = tr.CLIPVisionModelWithProjection(hc).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in R.module_state_dict(sd, cfg).items()}, strict=False)
    with torch.no_grad():
        out = m.double()(torch.from_numpy(pv).double(), output_hidden_states=True)
    r = R.forward(sd, cfg, pv)
    assert R.relerr(r["image_embeds"], out.image_embeds.numpy()) < 1e-12
    assert R.relerr(r["hidden_states"][-2], out.hidden_states[-2].numpy()) < 1e-12


# ------------------------------------------------------------------------------------------------ the checker
def test_checker_restatement_returns_fixture(gold):
    s = R.synth_safety()
    for k, v in s.items():
        assert np.array_equal(v, gold["safety_" + k]), k
    scores, flags = R.safety_check(s["embeds"], s["special_care_embeds"], s["concept_embeds"], s["special_care_embeds_weights"],
                                   s["concept_embeds_weights"])
    assert np.array_equal(flags, gold["safety_flags"]) and np.abs(scores - gold["safety_scores"]).max() < 1e-12
    assert list(flags) == [False, True, True, False]
    assert np.abs(scores - 0.0005).min() >= 1e-3          # no score near the decision boundary
    # Python's round(x, 3) > 0 is "exceeds 0.0005" for every stored score
    assert all((round(float(x), 3) > 0) == (float(x) > 0.0005) for x in scores.ravel())
    all_on = R.with_thresholds(s, -1.0)
    assert R.safety_check(s["embeds"], s["special_care_embeds"], s["concept_embeds"], all_on["special_care_embeds_weights"],
                          all_on["concept_embeds_weights"])[1].all()


# ------------------------------------------------------------------------------------------------ ABI mirrors
def test_struct_mirrors():
    assert C.sizeof(E.pd_clip_preprocess_args) == 8 + 8 * 4 + 8 + 6 * 4 + 4 * 4
    assert C.sizeof(E.pd_clip_vision_config) == 8 * 4 + 4 + 4 + 6 * 4 + 64 + 4 * 4
    assert C.sizeof(E.pd_clip_vision_args) == 16 + 6 * 4 + 3 * 8 + 2 * 8
    assert E.pd_clip_vision_args.image_embeds.offset == 40 and E.pd_clip_preprocess_args.dst.offset == 40
    for n in ("pd_clip_preprocess", "pd_clip_vision_configure", "pd_clip_vision_forward", "pd_safety_configure", "pd_safety_check",
              "pd_safety_blank", "pd_resample_coefficients_ex"):
        assert n in E.EXPORTS and hasattr(E.load_library(), n)
    assert W.CLIP_VIT_L14_SAFETY.prefix == "safety_checker.vision_model." and not W.CLIP_VIT_L14_SAFETY.stream_f32
    assert (W.CLIP_VIT_H14.hidden // W.CLIP_VIT_H14.heads, W.CLIP_VIT_H14.patches + 1, W.CLIP_VIT_H14.act) == (80, 257, "gelu")
    assert W.ModelConfig().clip_vision == () and not W.ModelConfig().safety_checker


# ------------------------------------------------------------------------------------------------ the pipeline's surface
class _StubEngine:
    """records every call; the checker flags by a rule on the pictures, the tower returns recognisable arrays"""
    cfg = W.TINY
    device = 0

    def __init__(self, flag_rule=lambda u8: u8.reshape(len(u8), -1).mean(1) > 127):
        self.calls = []
        self.flag_rule = flag_rule
        self._clip_vision = {E.SAFETY_PREFIX: R.CONFIGS["A"][0], E.IMAGE_ENCODER_PREFIX: R.CONFIGS["C"][0]}

    def safety_check(self, x, return_scores=False):
        self.calls.append(("safety_check", tuple(x.shape), str(x.dtype)))
        return np.asarray(self.flag_rule(np.asarray(x)))

    def clip_vision(self, x, what="embeds", hidden_layer=-2, prefix=None):
        self.calls.append(("clip_vision", tuple(x.shape), str(x.dtype), what, hidden_layer, prefix))
        cfg = self._clip_vision[prefix]
        B = x.shape[0]
        fill = float(np.asarray(x, np.float64).mean())
        if what == "hidden":
            return np.full((B, cfg.patches + 1, cfg.hidden), fill, np.float32)
        return np.arange(B * cfg.proj_dim, dtype=np.float32).reshape(B, cfg.proj_dim) + 1


def test_pipeline_without_checker_touches_nothing():
    eng = _StubEngine()
    pipe = PromptDiffusionPipeline(eng)
    assert pipe.safety_checker is None and pipe.image_encoder is None and pipe.requires_safety_checker is False
    img = np.random.default_rng(0).random((2, 16, 16, 3)).astype(np.float32)
    out, flags = pipe.run_safety_checker(img)
    assert out is img and flags is None and eng.calls == []
    with pytest.raises(ValueError, match="image_encoder"):
        pipe.encode_image(img, None, 1)
    with pytest.raises(ValueError, match="requires_safety_checker"):
        PromptDiffusionPipeline(eng, requires_safety_checker=True)
    with pytest.raises(ValueError, match="feature_extractor"):
        PromptDiffusionPipeline(eng, safety_checker=lambda images, clip_input: (images, [False]))
    with pytest.raises(NotImplementedError, match="ip_adapter_image"):
        PromptDiffusionPipeline(eng, safety_checker=True)(prompt_embeds=np.zeros((1, 77, 96), np.float32), ip_adapter_image=img,
                                                           negative_prompt_embeds=np.zeros((1, 77, 96), np.float32),
                                                           image=np.zeros((1, 64, 64, 3), np.float32),
                                                           image_pair=[np.zeros((1, 64, 64, 3), np.float32)] * 2)


def test_run_safety_checker_with_engine_and_callable():
    eng = _StubEngine()
    pipe = PromptDiffusionPipeline(eng, safety_checker=True)
    img = np.stack([np.full((16, 16, 3), 0.9, np.float32), np.full((16, 16, 3), 0.1, np.float32)])
    out, flags = pipe.run_safety_checker(img)
    assert flags == [True, False] and not out[0].any() and np.array_equal(out[1], img[1]) and img[0].all()   # input left alone
    assert eng.calls == [("safety_check", (2, 16, 16, 3), "uint8")]
    # a reduction the device preprocessing refuses goes through the caller's feature_extractor
    seen = {}

    class _FE:
        def __call__(self, pics, return_tensors=None):
            seen["n"], seen["rt"] = len(pics), return_tensors
            return type("R", (), {"pixel_values": np.zeros((len(pics), 3, 56, 56), np.float32)})()

    big = np.zeros((1, 56 * 9, 56 * 9, 3), np.float32)
    with pytest.raises(ValueError, match="feature_extractor"):
        pipe.run_safety_checker(big)
    pipe2 = PromptDiffusionPipeline(eng, safety_checker=True, feature_extractor=_FE())
    eng.flag_rule = lambda e: np.zeros(len(e), bool)
    _, flags = pipe2.run_safety_checker(big)
    assert flags == [False] and seen == {"n": 1, "rt": "np"} and eng.calls[-2][0] == "clip_vision" and eng.calls[-2][5] == E.SAFETY_PREFIX
    # an injected callable keeps precedence and diffusers' signature
    got = {}

    def checker(images, clip_input):
        got["shape"] = clip_input.shape
        return images, [True] * len(images)

    n = len(eng.calls)
    pipe3 = PromptDiffusionPipeline(eng, safety_checker=checker, feature_extractor=_FE(), requires_safety_checker=True)
    _, flags = pipe3.run_safety_checker(img)
    assert flags == [True, True] and got["shape"] == (2, 3, 56, 56) and len(eng.calls) == n


def test_encode_image_shapes_and_zero_negatives():
    eng = _StubEngine()
    pipe = PromptDiffusionPipeline(eng, image_encoder=True)
    cfg = R.CONFIGS["C"][0]
    pics = np.full((2, 40, 60, 3), 200, np.uint8)
    emb, neg = pipe.encode_image(pics, None, 3)
    assert emb.shape == neg.shape == (6, cfg.proj_dim) and not neg.any()
    assert np.array_equal(emb[0], emb[2]) and np.array_equal(emb[3], emb[5]) and not np.array_equal(emb[0], emb[3])   # repeat_interleave
    assert eng.calls == [("clip_vision", (2, 40, 60, 3), "uint8", "embeds", -2, E.IMAGE_ENCODER_PREFIX)]
    hid, unc = pipe.encode_image(pics, None, 2, output_hidden_states=True)
    assert hid.shape == unc.shape == (4, cfg.patches + 1, cfg.hidden)
    assert (hid == 200).all() and not unc.any()                   # the unconditional pass saw all-zero pixel_values
    assert eng.calls[-1] == ("clip_vision", (2, 3, cfg.image_size, cfg.image_size), "float32", "hidden", -2, E.IMAGE_ENCODER_PREFIX)
    pv = np.ones((1, 3, cfg.image_size, cfg.image_size), np.float32)
    emb, neg = pipe.encode_image(pv, None, 1)
    assert eng.calls[-1][1:3] == ((1, 3, cfg.image_size, cfg.image_size), "float32") and emb.shape == (1, cfg.proj_dim)


class _CallEngine(_StubEngine):
    """... plus what __call__ itself touches on the fused DDIM path: the loop and the first stage, as recorded stand-ins"""

    def __init__(self, hw=64, bright=(0.9, -0.9), **kw):
        super().__init__(**kw)
        self.hw, self.bright = hw, bright

    def num_ddim_steps(self, n):
        return n

    def ddim_sample(self, **kw):
        self.calls.append(("ddim_sample",))
        B = kw["x_T"].shape[0]
        return np.ones((B, 4, self.hw // 8, self.hw // 8), np.float32)

    def vae_weights_missing(self):
        return 0

    def vae_decode(self, lat):
        self.calls.append(("vae_decode",))
        B = lat.shape[0]
        return np.stack([np.full((3, self.hw, self.hw), self.bright[i % 2], np.float32) for i in range(B)])     # in [-1, 1]


def _call_kw(B=2, hw=64):
    emb = np.zeros((B, 77, 96), np.float32)
    img = np.zeros((B, hw, hw, 3), np.float32)
    return dict(prompt_embeds=emb, negative_prompt_embeds=emb, image=img, image_pair=[img.copy(), img.copy()], num_inference_steps=2,
                latents=np.zeros((B, 4, hw // 8, hw // 8), np.float32))


def test_call_without_checker_makes_no_new_engine_call(device_images=False):
    logs = []
    for extra in ({}, dict(safety_checker=None, feature_extractor=None, image_encoder=None, requires_safety_checker=False)):
        eng = _CallEngine()
        pipe = PromptDiffusionPipeline(eng, device_images=device_images, **extra)
        out = pipe(output_type="np", **_call_kw())
        assert out.nsfw_content_detected is None and out.images.shape == (2, 64, 64, 3) and out.images[0].any()
        assert pipe(output_type="np", return_dict=False, **_call_kw())[1] is None
        assert pipe(output_type="latent", **_call_kw()).nsfw_content_detected is None
        logs.append(list(eng.calls))
    assert logs[0] == logs[1] and {c[0] for c in logs[0]} == {"ddim_sample", "vae_decode"}


def test_call_with_checker_never_returns_unchecked_pictures(device_images=False):
    """every way a checker can be set ends in checked pictures: the engine's, the engine's on pictures the device preprocessing
    refuses, and a callable (tests/test_safety_pipeline_gpu.py repeats the last two with the image ends on the device)"""
    class _FE:
        def __call__(self, pics, return_tensors=None):
            return type("R", (), {"pixel_values": np.stack([np.full((3, 56, 56), np.asarray(p).mean() / 255, np.float32) for p in pics])})()

    # the engine's checker on 64 x 64: the stub flags the bright picture
    eng = _CallEngine()
    out = PromptDiffusionPipeline(eng, device_images=device_images, safety_checker=True)(output_type="pil", **_call_kw())
    assert out.nsfw_content_detected == [True, False]
    assert not np.asarray(out.images[0]).any() and np.asarray(out.images[1]).any() and ("safety_check", (2, 64, 64, 3), "uint8") in eng.calls
    # ... on 512 x 512 with a 56-pixel tower: a 9.1 x reduction goes through the caller's feature_extractor, and is still checked
    eng = _CallEngine(hw=512, flag_rule=lambda e: np.arange(len(e)) == 0)      # (the stub's embeddings say nothing: flag the first)
    assert not E.clip_preprocess_supported(512, 512, 56)
    out = PromptDiffusionPipeline(eng, device_images=device_images, safety_checker=True, feature_extractor=_FE())(output_type="pil", **_call_kw(hw=512))
    assert out.nsfw_content_detected == [True, False] and not np.asarray(out.images[0]).any() and np.asarray(out.images[1]).any()
    assert [c[0] for c in eng.calls if c[0] in ("clip_vision", "safety_check")] == ["clip_vision", "safety_check"]
    # a callable with diffusers' signature keeps precedence over the engine's checker, device_images or not, and its flagged pictures
    # come back black even if it leaves them as they are
    seen = []

    def checker(images, clip_input):
        seen.append((images.shape, clip_input.shape))
        return images, [bool(clip_input[i].mean() > 0.5) for i in range(len(images))]

    eng = _CallEngine()
    pipe = PromptDiffusionPipeline(eng, device_images=device_images, safety_checker=checker, feature_extractor=_FE(), requires_safety_checker=True)
    out = pipe(output_type="pil", **_call_kw())
    assert out.nsfw_content_detected == [True, False] and seen == [((2, 64, 64, 3), (2, 3, 56, 56))]
    assert not np.asarray(out.images[0]).any() and np.asarray(out.images[1]).any()
    assert not any(c[0] in ("safety_check", "clip_vision") for c in eng.calls)
    imgs, flags = pipe(output_type="np", return_dict=False, **_call_kw())
    assert flags == [True, False] and not imgs[0].any() and imgs[1].any()


def test_uint8_tensors_are_pictures():
    torch = pytest.importorskip("torch")
    eng = _StubEngine()
    pics = np.full((2, 40, 60, 3), 200, np.uint8)
    got = PromptDiffusionPipeline._pictures_u8(torch.from_numpy(pics))
    assert got.dtype == np.uint8 and np.array_equal(got, pics)
    PromptDiffusionPipeline(eng, image_encoder=True).encode_image(torch.from_numpy(pics), None, 1)
    assert eng.calls[-1][:3] == ("clip_vision", (2, 40, 60, 3), "uint8")
    _, flags = PromptDiffusionPipeline(eng, safety_checker=True).run_safety_checker(torch.from_numpy(pics))
    assert flags == [True, True] and eng.calls[-1] == ("safety_check", (2, 40, 60, 3), "uint8")
