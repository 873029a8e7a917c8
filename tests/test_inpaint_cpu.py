"""img2img / inpainting on the host side (CPU only): the pd_sample_args layout, get_timesteps, the mask processor, argument
checks that run before the engine is touched, the fused-UniPC arguments of a truncated grid, and the proof that the fused
UniPC rows of a truncated grid are diffusers' set_begin_index stepping."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import weights as W
from prompt_diffusion_amd.pipeline import (PromptDiffusionImg2ImgPipeline, PromptDiffusionInpaintPipeline,
                                           PromptDiffusionPipeline, add_noise_coefficients)
from prompt_diffusion_amd.schedulers import UniPCMultistepScheduler

from tests import inpaint_ref as R
from tests.test_unipc_fused_cpu import fake_eps, run_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(E.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return E.load_library()


class _NoEngine:
    cfg = W.TINY

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} touched before input validation finished")


def _kw(b=1, hw=64):
    img = np.zeros((b, hw, hw, 3), np.float32)
    emb = np.zeros((b, 77, 96), np.float32)
    return dict(prompt_embeds=emb, negative_prompt_embeds=emb, control_image=img, image_pair=[img, img.copy()])


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_sample_args_layout():
    f = E.pd_sample_args
    ts = f.timesteps.offset
    assert (f.init_latents.offset, f.mask.offset, f.init_flags.offset, f.reserved.offset) == (ts + 8, ts + 16, ts + 24, ts + 28)
    # the six reserved ints of ABI 2 became the new fields: the size is unchanged
    assert C.sizeof(f) == ts + 8 + 6 * 4 == 160
    assert f.reserved.size == 4
    assert E.PD_INIT_PURE_NOISE == 1
    hdr = open(os.path.join(ROOT, "include", "pdengine.h")).read()
    for decl in ("const float* init_latents;", "const float* mask;", "int32_t init_flags;", "#define PD_INIT_PURE_NOISE 1",
                 "#define PD_ABI_VERSION 2"):
        assert decl in hdr, decl


def test_abi_version_unchanged(lib):
    assert lib.pd_abi_version() == 2


# ---------------------------------------------------------------------------------------------------------------- grid
@pytest.mark.parametrize("S,strength", [(50, 0.8), (50, 1.0), (50, 0.6), (20, 0.75), (10, 0.15), (7, 0.5), (5, 0.2), (3, 0.99)])
def test_get_timesteps_truncation(S, strength):
    pipe = PromptDiffusionPipeline(_NoEngine())
    full = list(range(999, 999 - 10 * S, -10))
    grid, k = pipe.get_timesteps(full, strength)
    init = min(int(S * strength), S)
    assert k == S - init and grid == full[S - init:] and len(grid) == init
    assert (grid, k) == R.get_timesteps(full, strength)
    # a scheduler with set_begin_index learns the index
    sched = UniPCMultistepScheduler()
    sched.set_timesteps(S)
    pipe = PromptDiffusionPipeline(_NoEngine(), scheduler=sched)
    grid, k = pipe.get_timesteps(list(sched.timesteps), strength)
    assert sched._step_index == k and grid == [int(t) for t in sched.timesteps[k:]]


def test_get_timesteps_no_step_left():
    pipe = PromptDiffusionPipeline(_NoEngine())
    for S, strength in ((50, 0.0), (10, 0.05), (3, 0.3)):
        with pytest.raises(ValueError, match="which is < 1 and not appropriate"):
            pipe.get_timesteps(list(range(S, 0, -1)), strength)


def test_add_noise_coefficients_table():
    ts = [981, 500, 21, 1, 0]
    sa, sb = add_noise_coefficients(W.SD15, ts)
    ac = R.alphas_cumprod_f32(W.SD15)
    assert sa.dtype == np.float32 and sb.dtype == np.float32
    np.testing.assert_array_equal(sa, np.sqrt(ac[ts]))
    np.testing.assert_array_equal(sb, np.sqrt(np.float32(1.0) - ac[ts]))


# ---------------------------------------------------------------------------------------------------------------- mask
def test_mask_processing_pil_and_arrays():
    from PIL import Image
    pipe = PromptDiffusionPipeline(_NoEngine())
    rng = np.random.default_rng(3)
    m01 = rng.uniform(0, 1, (32, 48)).astype(np.float32)
    # arrays at the image size: binarize at 0.5, pixel (8i, 8j), repeated to the batch
    got = pipe.prepare_mask(m01, 48, 32, 3)
    assert got.shape == (3, 1, 4, 6) and got.dtype == np.float32
    np.testing.assert_array_equal(got, R.process_mask(m01[None, None], 3))
    np.testing.assert_array_equal(got[1, 0], (m01[::8, ::8] >= 0.5).astype(np.float32))
    np.testing.assert_array_equal(pipe.prepare_mask(m01[None], 48, 32, 2), R.process_mask(m01[None, None], 2))
    np.testing.assert_array_equal(pipe.prepare_mask(m01[:, :, None], 48, 32, 1), R.process_mask(m01[None, None], 1))
    two = np.stack([m01, 1 - m01])
    np.testing.assert_array_equal(pipe.prepare_mask(two[..., None], 48, 32, 4), R.process_mask(two[:, None], 4))
    assert np.array_equal(pipe.prepare_mask(two[..., None], 48, 32, 4)[2], pipe.prepare_mask(m01, 48, 32, 1)[0])   # tiled
    # PIL: grayscale, LANCZOS resize to the image size, then the same
    pil = Image.fromarray((rng.uniform(0, 1, (16, 24, 3)) * 255).astype("uint8"))
    ref = np.asarray(pil.convert("L").resize((48, 32), resample=Image.LANCZOS), np.float32) / 255.0
    np.testing.assert_array_equal(pipe.prepare_mask(pil, 48, 32, 2), R.process_mask(ref[None, None], 2))
    with pytest.raises(ValueError, match="is 40x32"):
        pipe.prepare_mask(np.zeros((32, 40), np.float32), 48, 32, 1)
    with pytest.raises(ValueError, match="duplicate"):
        pipe.prepare_mask(two, 48, 32, 3)


# ---------------------------------------------------------------------------------------------------------------- checks
def test_argument_errors_before_the_engine():
    inp = PromptDiffusionInpaintPipeline(_NoEngine())
    i2i = PromptDiffusionImg2ImgPipeline(_NoEngine())
    kw = _kw()
    lat = np.zeros((1, 4, 8, 8), np.float32)
    mask = np.ones((64, 64), np.float32)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="strength should in"):
            i2i(image=lat, strength=bad, **kw)
        with pytest.raises(ValueError, match="strength should in"):
            inp(image=lat, mask_image=mask, strength=bad, **kw)
    with pytest.raises(ValueError, match="mask_image"):
        inp(image=lat, **kw)
    with pytest.raises(ValueError, match="init image"):
        i2i(**kw)
    with pytest.raises(TypeError, match="mask_image"):
        inp(image=lat, mask_image="mask.png", **kw)
    with pytest.raises(TypeError, match="init image"):
        i2i(image=3, **kw)
    with pytest.raises(ValueError, match="is 32x32"):
        inp(image=lat, mask_image=np.ones((32, 32), np.float32), **kw)
    with pytest.raises(ValueError, match=r"latent `image` must be"):
        i2i(image=np.zeros((1, 4, 4, 4), np.float32), **kw)
    with pytest.raises(NotImplementedError):
        inp(image=lat, mask_image=mask, padding_mask_crop=8, **kw)
    with pytest.raises(TypeError, match="image must be passed"):        # the control image is still checked first
        i2i(image=lat, **dict(kw, control_image=None))


def test_pixel_image_needs_the_vae_encoder():
    class _NoEncoder(_NoEngine):
        cfg = W.TINY          # vae_encoder off

    i2i = PromptDiffusionImg2ImgPipeline(_NoEncoder())
    with pytest.raises(ValueError, match="VAE encoder"):
        i2i(image=np.zeros((1, 64, 64, 3), np.float32), **_kw())


class _Recorder:
    """records what the pipeline hands to the engine's loops (no GPU)"""
    cfg = W.TINY

    def __init__(self):
        self.calls = []

    def num_ddim_steps(self, steps):
        return len(range(0, self.cfg.timesteps, self.cfg.timesteps // steps))

    def make_schedule(self, steps, eta=0.0):
        return dict(ddim_timesteps=np.arange(0, self.cfg.timesteps, self.cfg.timesteps // steps) + 1)

    def _out(self, name, kw):
        self.calls.append((name, kw))
        return np.zeros_like(kw["x_T"])

    def ddim_sample(self, **kw):
        return self._out("ddim", kw)

    def unipc_sample(self, **kw):
        return self._out("unipc", kw)


def test_engine_arguments_of_a_truncated_grid():
    rng = np.random.default_rng(0)
    z0 = rng.standard_normal((2, 4, 8, 8)).astype(np.float32)
    eps = rng.standard_normal((2, 4, 8, 8)).astype(np.float32)
    mask = np.zeros((64, 64), np.float32)
    mask[:, 32:] = 1.0
    kw = dict(_kw(b=2), latents=eps, output_type="latent")
    # default DDIM: the tail of the LDM grid as custom timesteps, z0 / eps / mask to the engine
    eng = _Recorder()
    PromptDiffusionInpaintPipeline(eng)(image=z0, mask_image=mask, strength=0.5, num_inference_steps=10, **kw)
    name, a = eng.calls[-1]
    assert name == "ddim" and a["timesteps"] == [401, 301, 201, 101, 1]
    np.testing.assert_array_equal(a["init_latents"], z0)
    np.testing.assert_array_equal(a["x_T"], eps)
    np.testing.assert_array_equal(a["mask"][:, 0, :, 4:], 1.0)
    assert a["mask"].shape == (2, 1, 8, 8) and not a["mask"][:, :, :, :4].any()
    assert a["init_pure_noise"] is True            # given latents: they are the start
    assert a["control_scales_step"].shape == (5, E.PD_NUM_CONTROL)
    PromptDiffusionImg2ImgPipeline(eng)(image=z0, strength=0.5, num_inference_steps=10, **kw)
    name, a = eng.calls[-1]
    assert a["mask"] is None and a["init_pure_noise"] is False
    # fused UniPC: the tail of the scheduler's grid, disable_corrector shifted by -t_start
    sched = UniPCMultistepScheduler(solver_order=3, disable_corrector=[1, 4, 6])
    pipe = PromptDiffusionInpaintPipeline(eng, scheduler=sched, fuse_scheduler=True)
    pipe(image=z0, mask_image=mask, strength=0.6, num_inference_steps=10, **dict(kw, latents=None), generator=np.random.default_rng(1))
    name, a = eng.calls[-1]
    assert name == "unipc" and a["timesteps"] == [int(t) for t in sched.timesteps[4:]]
    assert a["disable_corrector"] == [0, 2] and a["order"] == 3
    assert a["init_pure_noise"] is False
    np.testing.assert_array_equal(a["x_T"], np.random.default_rng(1).standard_normal((2, 4, 8, 8), dtype=np.float32))


# ---------------------------------------------------------------------------------------------------------------- begin index
def test_set_begin_index_matches_fused_rows_of_the_tail(lib):
    """UniPCMultistepScheduler.set_begin_index(k), stepping timesteps[k:], against the fused coefficient rows of the grid
    timesteps[k:] with disable_corrector shifted by -k, applied by the device kernel's update in NumPy."""
    x_T = np.random.default_rng(4).standard_normal((2, 4, 4, 4))
    worst, n = 0.0, 0
    for order, st, dc, steps, k in itertools.product((1, 2, 3), ("bh1", "bh2"), ((), (1,), (0, 3, 5), (6, 7)), (8, 20),
                                                     (1, 3, 5)):
        sc = UniPCMultistepScheduler(solver_order=order, solver_type=st, disable_corrector=list(dc))
        sc.set_timesteps(steps)
        sc.set_begin_index(k)
        x, ref = x_T, []
        for t in sc.timesteps[k:]:
            x = sc.step(fake_eps(x, int(t)), t, x, return_dict=False)[0]
            ref.append(x)
        coef = E.unipc_coefficients(W.TINY, sc.timesteps[k:], order=order, solver_type=st,
                                    disable_corrector=[d - k for d in dc if d >= k])
        got = run_rows(coef, sc.timesteps[k:], x_T)
        assert len(got) == len(ref) == steps - k
        for i, (g, r) in enumerate(zip(got, ref)):
            err = float(np.abs(g - r).max() / np.abs(r).max())
            assert err <= 1e-10, (order, st, dc, steps, k, i, err)
            worst = max(worst, err)
        n += 1
    print(f"max relative error over {n} variants: {worst:.3e}")


def test_set_begin_index_resets_and_checks():
    sc = UniPCMultistepScheduler()
    sc.set_timesteps(6)
    x = np.ones((1, 4, 2, 2))
    for t in sc.timesteps[:2]:
        x = sc.step(fake_eps(x, int(t)), t, x, return_dict=False)[0]
    sc.set_begin_index(3)
    assert sc._step_index == 3 and sc.last_sample is None and sc.lower_order_nums == 0
    with pytest.raises(ValueError, match="expects timestep"):
        sc.step(x, sc.timesteps[0], x)
    with pytest.raises(ValueError, match="begin_index"):
        sc.set_begin_index(6)
