"""FreeU on the host side: the closed form the kernel computes against the FFT restatement of diffusers' fourier_filter, the
FreeU-aware oracle UNet against pd_oracle with FreeU off, and the pipeline / engine API surface."""
import inspect
import os
import re

import numpy as np
import pytest

from oracle import pd_oracle as O
from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import weights as W
from prompt_diffusion_amd.pipeline import PromptDiffusionPipeline
from tests import freeu_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 3), (3, 1), (2, 2), (3, 2), (3, 3), (4, 4), (6, 4), (8, 8), (9, 7), (12, 12), (16, 16)]


@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("scale", [0.9, 0.2, 1.0, 1.7])
def test_closed_form_matches_fft(hw, scale):
    rng = np.random.default_rng(hw[0] * 31 + hw[1])
    x = rng.standard_normal((2, 3) + hw).astype(np.float32)
    ref = FR.fourier_filter(x, 1, scale)
    got = FR.freeu_closed_form(x, scale)
    assert np.abs(got - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max())
    if scale == 1.0:
        np.testing.assert_allclose(got, x, rtol=0, atol=1e-6)


def test_band_is_frequencies_zero_and_minus_one():
    """After fftshift, the [H//2-1 : H//2+1] slice (Python rules) holds the frequencies {-1, 0}; only 0 when H == 1."""
    for n in range(1, 12):
        freqs = np.fft.fftshift(np.round(np.fft.fftfreq(n) * n).astype(int))
        band = sorted(freqs[n // 2 - 1:n // 2 + 1].tolist())
        assert band == ([0] if n == 1 else [-1, 0]), (n, band)


def test_apply_freeu_scales_half_the_backbone():
    rng = np.random.default_rng(1)
    h = rng.standard_normal((2, 8, 4, 4)).astype(np.float32)
    skip = rng.standard_normal((2, 6, 4, 4)).astype(np.float32)
    h1, s1 = FR.apply_freeu(0, h, skip, 0.9, 0.2, 1.5, 1.6)
    np.testing.assert_array_equal(h1[:, :4], h[:, :4] * np.float32(1.5))
    np.testing.assert_array_equal(h1[:, 4:], h[:, 4:])
    np.testing.assert_array_equal(s1, FR.fourier_filter(skip, 1, 0.9))
    h2, _ = FR.apply_freeu(1, h, skip, 0.9, 0.2, 1.5, 1.6)
    np.testing.assert_array_equal(h2[:, :4], h[:, :4] * np.float32(1.6))


@pytest.fixture(scope="module")
def tiny_unet_inputs():
    cfg = W.TINY
    sd = W.synth_state_dict(cfg)
    lay = O.make_layouts(cfg, W)
    inp = W.synth_inputs(cfg, 1, 8, 8, seed=5)
    x = np.concatenate([inp["x_T"]] * 2)
    t = np.array([801, 801], np.int64)
    ctx = np.concatenate([inp["ctx_uncond"], inp["ctx_cond"]])
    ctl = O.controlnet_forward(sd, cfg, lay, x, t, np.concatenate([inp["pair"]] * 2), np.concatenate([inp["query"]] * 2), ctx)
    return cfg, sd, lay, x, t, ctx, ctl


def test_oracle_unet_off_is_bit_identical(tiny_unet_inputs):
    cfg, sd, lay, x, t, ctx, ctl = tiny_unet_inputs
    ref = O.controlled_unet_forward(sd, cfg, lay, x, t, ctx, ctl)
    for fu in (None, (0.0, 0.0, 0.0, 0.0), (0.9, 0.2, 0.0, 1.6), (0.0, 0.2, 1.5, 1.6)):
        np.testing.assert_array_equal(FR.controlled_unet_forward(sd, cfg, lay, x, t, ctx, ctl, freeu=fu), ref)
    ref_mid = O.controlled_unet_forward(sd, cfg, lay, x, t, ctx, ctl, only_mid_control=True)
    np.testing.assert_array_equal(FR.controlled_unet_forward(sd, cfg, lay, x, t, ctx, ctl, True, None), ref_mid)
    on = FR.controlled_unet_forward(sd, cfg, lay, x, t, ctx, ctl, freeu=(0.9, 0.2, 1.5, 1.6))
    assert np.abs(on - ref).max() > 1e-2 * np.abs(ref).max()
    # the context manager routes pd_oracle's apply_model through the FreeU UNet and restores it afterwards
    with FR.enabled(0.9, 0.2, 1.5, 1.6):
        np.testing.assert_array_equal(O.controlled_unet_forward(sd, cfg, lay, x, t, ctx, ctl), on)
    np.testing.assert_array_equal(O.controlled_unet_forward(sd, cfg, lay, x, t, ctx, ctl), ref)


class _RecordingEngine:
    cfg = W.TINY

    def __init__(self):
        self.calls = []

    def set_freeu(self, s1, s2, b1, b2):
        self.calls.append(("set", s1, s2, b1, b2))

    def disable_freeu(self):
        self.calls.append(("disable",))


def test_pipeline_forwards_freeu():
    eng = _RecordingEngine()
    pipe = PromptDiffusionPipeline(eng)
    pipe.enable_freeu(s1=0.9, s2=0.2, b1=1.5, b2=1.6)
    pipe.enable_freeu(0.8, 0.3, 1.4, 1.5)
    pipe.disable_freeu()
    assert eng.calls == [("set", 0.9, 0.2, 1.5, 1.6), ("set", 0.8, 0.3, 1.4, 1.5), ("disable",)]
    assert list(inspect.signature(PromptDiffusionPipeline.enable_freeu).parameters) == ["self", "s1", "s2", "b1", "b2"]
    assert "arxiv.org/abs/2309.11497" in PromptDiffusionPipeline.enable_freeu.__doc__
    assert list(inspect.signature(PromptDiffusionPipeline.disable_freeu).parameters) == ["self"]


def test_c_abi_declares_freeu():
    h = open(os.path.join(ROOT, "include", "pdengine.h")).read()
    ops = open(os.path.join(ROOT, "include", "pdengine_ops.h")).read()
    assert re.search(r"int pd_set_freeu\(pd_engine\* e, float s1, float s2, float b1, float b2\);", h)
    assert re.search(r"int pd_get_freeu\(pd_engine\* e, float out\[4\]\);", h)
    assert "int pd_op_freeu_concat(" in ops
    for n in ("pd_set_freeu", "pd_get_freeu", "pd_op_freeu_concat"):
        assert n in E.EXPORTS
    assert callable(getattr(E.Engine, "set_freeu")) and callable(getattr(E.Engine, "disable_freeu"))
    assert isinstance(inspect.getattr_static(E.Engine, "freeu"), property)
