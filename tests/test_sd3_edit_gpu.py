"""SD3 img2img and inpainting inside the engine's flow-matching loop (pd_sd3_sample_ex, SD3Engine.sample(init_latents=, mask=, noise=,
from_seed=), the Img2Img / Inpaint pipelines) against tests/sd3_edit_ref.py: the NumPy float32 restatement of the start state and the
blend around oracle/sd3_oracle.py forwards.  Parity with diffusers is unpinned, like the rest of the SD3 path."""
import ctypes as C

import numpy as np
import pytest

from oracle import sd3_oracle as O
from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import sd3
from prompt_diffusion_amd.pipeline import EngineGenerator
from prompt_diffusion_amd.pipeline_sd3 import StableDiffusion3PromptDiffusionImg2ImgPipeline as Img2Img
from prompt_diffusion_amd.pipeline_sd3 import StableDiffusion3PromptDiffusionInpaintPipeline as Inpaint
from prompt_diffusion_amd.pipeline_sd3 import StableDiffusion3PromptDiffusionPipeline as Pipe
from tests import sd3_edit_ref as R

pytestmark = pytest.mark.gpu
CFG = sd3.SD3_TINY
STEPS, GUIDE = 4, 5.0


def relerr(a, b):
    return float(np.abs(np.asarray(a) - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def sd():
    return sd3.synth_sd3_state_dict(CFG)


@pytest.fixture(scope="module")
def eng(sd):
    e = sd3.SD3Engine(CFG, precision="f32")
    e.load_state_dict(sd)
    yield e
    e.close()


def arrays(B, h, w, S, seed):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    c = CFG.in_channels
    a = dict(eps=f(B, c, h, w), z0=f(B, c, h, w), cond=f(B, c, h, w), pair=f(B, c, h, w), pe=f(B, S, CFG.joint_dim), npe=f(B, S, CFG.joint_dim),
             ppe=f(B, CFG.pooled_dim), nppe=f(B, CFG.pooled_dim))
    # the pixel mask (8 pixels per latent pixel): a region that differs per sample and is neither row- nor column-symmetric
    m = np.zeros((B, 8 * h, 8 * w), np.float32)
    for b in range(B):
        m[b, 8 * (1 + b):8 * (h - 2), 8 * 2:8 * (w - 1 - b)] = 1.0
    a["mask_px"], a["mask"] = m, np.ascontiguousarray(m[:, None, ::8, ::8])
    return a


def pipe_kw(a, **over):
    kw = dict(prompt_embeds=a["pe"], pooled_prompt_embeds=a["ppe"], negative_prompt_embeds=a["npe"], negative_pooled_prompt_embeds=a["nppe"],
              control_image=a["cond"], control_image_pair=a["pair"], num_inference_steps=STEPS, guidance_scale=GUIDE, output_type="latent")
    kw.update(over)
    return kw


def ref_loop(sd, a, strength, mask=None, guidance=GUIDE, steps=STEPS, **kw):
    vel = R.oracle_velocity(sd, CFG, a["pe"], a["npe"], a["ppe"], a["nppe"], a["cond"], a["pair"], guidance)
    return R.sample(vel, R.truncate(O.flow_match_sigmas(steps), strength), a["z0"], a["eps"], mask=mask, **kw)


def test_img2img_and_inpaint_against_the_restated_loop(eng, sd):
    a = arrays(1, 8, 8, 6, 1)
    out = Img2Img(eng)(image=a["z0"], strength=0.5, latents=a["eps"], **pipe_kw(a))["images"]
    assert out.shape == a["z0"].shape and relerr(out, ref_loop(sd, a, 0.5)) < 6e-4
    pipe = Inpaint(eng)
    out = pipe(image=a["z0"], mask_image=a["mask_px"], strength=1.0, latents=a["eps"], **pipe_kw(a))["images"]
    assert relerr(out, ref_loop(sd, a, 1.0, a["mask"])) < 6e-4 and pipe.num_timesteps == STEPS
    keep = np.broadcast_to(a["mask"] == 0.0, out.shape)
    assert keep.any() and not keep.all() and np.array_equal(out[keep], a["z0"][keep])        # kept pixels hold z0 exactly at the end
    # B = 2 on a non-square grid, guidance off, inpainting at strength 0.75 (3 of 4 steps)
    a = arrays(2, 8, 12, 5, 2)
    out = pipe(image=a["z0"], mask_image=a["mask_px"], strength=0.75, latents=a["eps"], **pipe_kw(a, guidance_scale=1.0))["images"]
    assert relerr(out, ref_loop(sd, a, 0.75, a["mask"], guidance=1.0)) < 6e-4 and pipe.num_timesteps == 3
    keep = np.broadcast_to(a["mask"] == 0.0, out.shape)
    assert np.array_equal(out[keep], a["z0"][keep])


def test_bit_exact_identities(eng):
    a = arrays(2, 8, 12, 4, 3)
    kw = pipe_kw(a)
    plain = Pipe(eng)(latents=a["eps"], **kw)["images"]
    img = Img2Img(eng)(image=a["z0"], strength=1.0, latents=a["eps"], **kw)["images"]
    assert np.array_equal(img, plain)                 # sigma_0 = 1: the start state is eps and the update is the plain loop's
    ones = Inpaint(eng)(image=a["z0"], mask_image=np.ones_like(a["mask_px"]), strength=1.0, latents=a["eps"], **kw)["images"]
    assert np.array_equal(ones, img)
    half = Img2Img(eng)(image=a["z0"], strength=0.5, latents=a["eps"], **kw)["images"]
    ones = Inpaint(eng)(image=a["z0"], mask_image=np.ones_like(a["mask_px"]), strength=0.5, latents=a["eps"], **kw)["images"]
    assert np.array_equal(ones, half) and not np.array_equal(half, img)
    zeros = Inpaint(eng)(image=a["z0"], mask_image=np.zeros_like(a["mask_px"]), strength=0.5, latents=a["eps"], **kw)["images"]
    assert np.array_equal(zeros, a["z0"])
    # the engine call itself: `noise` and `latents` name the same eps; guidance off takes the undoubled path
    e_kw = dict(control_latents=a["cond"], pair_latents=a["pair"], num_inference_steps=STEPS, guidance_scale=1.0)
    p0 = eng.sample(a["eps"], a["pe"], a["ppe"], **e_kw)
    p1 = eng.sample(a["eps"], a["pe"], a["ppe"], init_latents=a["z0"], **e_kw)
    p2 = eng.sample(None, a["pe"], a["ppe"], init_latents=a["z0"], noise=a["eps"], **e_kw)
    assert np.array_equal(p0, p1) and np.array_equal(p1, p2)


def test_control_guidance_end_acts_on_the_truncated_steps(eng, sd):
    """strength 0.5 keeps steps 2, 3 of 4.  control_guidance_end = 0.5 over the remaining two steps keeps the ControlNet on the first of
    them alone; counted over the untruncated four it would be on at both (local indices 0, 1 of 4) or off at both (global indices 2, 3).
    The three loops differ by far more than the bound, so the check tells them apart."""
    a = arrays(1, 8, 8, 5, 4)
    out = Img2Img(eng)(image=a["z0"], strength=0.5, latents=a["eps"], control_guidance_end=0.5, **pipe_kw(a))["images"]
    want = ref_loop(sd, a, 0.5, guidance_end=0.5)
    both_off, both_on = ref_loop(sd, a, 0.5, guidance_end=0.0), ref_loop(sd, a, 0.5, guidance_end=1.0)
    assert relerr(both_off, want) > 6e-3 and relerr(both_on, want) > 6e-3
    assert relerr(out, want) < 6e-4


def test_callback_path_matches_the_fused_loop(eng):
    a = arrays(1, 8, 8, 4, 5)
    seen = []
    for pipe, extra in ((Img2Img(eng), {}), (Inpaint(eng), {"mask_image": a["mask_px"]})):
        kw = pipe_kw(a, image=a["z0"], strength=0.75, latents=a["eps"], control_guidance_end=0.67, **extra)
        fused = pipe(**kw)["images"]
        stepwise = pipe(callback_on_step_end=lambda p, i, t, k: seen.append(i) or {}, **kw)["images"]
        assert relerr(stepwise, fused) < 1e-5
    assert seen == [0, 1, 2, 0, 1, 2]
    keep = np.broadcast_to(a["mask"] == 0.0, stepwise.shape)
    assert np.array_equal(stepwise[keep], a["z0"][keep])


def test_engine_generator_equals_explicit_noise_from_randn(eng):
    a = arrays(2, 8, 12, 4, 6)
    shape = a["z0"].shape
    for pipe, extra in ((Img2Img(eng), {}), (Inpaint(eng), {"mask_image": a["mask_px"]})):
        kw = pipe_kw(a, image=a["z0"], strength=0.75, **extra)
        seeded = pipe(generator=EngineGenerator(77, sample_base=3), **kw)["images"]
        assert eng.rng == (77, 3)
        explicit = pipe(latents=eng.randn(shape, "xt", 0), **kw)["images"]
        assert np.array_equal(seeded, explicit)
        # the host-driven path draws the same numbers
        stepwise = pipe(generator=EngineGenerator(77, sample_base=3), callback_on_step_end=lambda p, i, t, k: {}, **kw)["images"]
        assert relerr(stepwise, seeded) < 1e-5
        # the second sample alone, as the shard that starts at global index 4 draws it (another batch size may sum in another
        # order; another draw would differ at order 1)
        one = {k: (v[1:] if isinstance(v, np.ndarray) and v.shape[0] == 2 else v) for k, v in kw.items()}
        shard = pipe(generator=EngineGenerator(77, sample_base=4), **one)["images"]
        assert relerr(shard, seeded[1:]) < 1e-4
    # without init_latents the seed flag draws the start latents themselves: the plain pipeline under an EngineGenerator
    plain = Pipe(eng)(generator=EngineGenerator(5), **pipe_kw(a))["images"]
    e_kw = dict(control_latents=a["cond"], pair_latents=a["pair"], num_inference_steps=STEPS, guidance_scale=GUIDE)
    drawn = eng.sample(None, a["pe"], a["ppe"], a["npe"], a["nppe"], from_seed=True, **e_kw)
    assert np.array_equal(drawn, plain)
    assert np.array_equal(drawn, eng.sample(eng.randn(shape, "xt", 0), a["pe"], a["ppe"], a["npe"], a["nppe"], **e_kw))
    eng.set_rng(0, 0)


def test_argument_errors(eng):
    a = arrays(1, 8, 8, 4, 7)
    kw = pipe_kw(a, latents=a["eps"])
    with pytest.raises(ValueError, match="strength"):
        Img2Img(eng)(image=a["z0"], strength=1.5, **kw)
    with pytest.raises(ValueError, match="steps"):
        Img2Img(eng)(image=a["z0"], strength=0.0, **kw)
    with pytest.raises(ValueError, match="must be passed"):
        Img2Img(eng)(**kw)
    with pytest.raises(ValueError, match="must be passed"):
        Inpaint(eng)(image=a["z0"], **kw)
    with pytest.raises(ValueError, match="latents must be"):
        Img2Img(eng)(image=a["z0"][:, :, :4], **kw)
    with pytest.raises(ValueError, match="mask_image is"):
        Inpaint(eng)(image=a["z0"], mask_image=a["mask_px"][:, :32], **kw)
    with pytest.raises(ValueError, match="vae_encode"):
        Img2Img(eng)(image=np.zeros((1, 64, 64, 3), np.float32), **kw)
    s_kw = dict(control_latents=a["cond"], pair_latents=a["pair"], num_inference_steps=2, guidance_scale=1.0)
    with pytest.raises(ValueError, match="needs `init_latents`"):
        eng.sample(a["eps"], a["pe"], a["ppe"], mask=a["mask"], **s_kw)
    with pytest.raises(ValueError, match="needs `init_latents`"):
        eng.sample(a["eps"], a["pe"], a["ppe"], noise=a["eps"], **s_kw)
    with pytest.raises(ValueError, match="from_seed"):
        eng.sample(a["eps"], a["pe"], a["ppe"], init_latents=a["z0"], from_seed=True, **s_kw)
    with pytest.raises(ValueError, match="noise is required"):
        eng.sample(None, a["pe"], a["ppe"], init_latents=a["z0"], **s_kw)
    with pytest.raises(ValueError, match="`mask` must be"):
        eng.sample(a["eps"], a["pe"], a["ppe"], init_latents=a["z0"], mask=a["mask"][..., :4], **s_kw)
    with pytest.raises(ValueError, match="`init_latents` must be"):
        eng.sample(a["eps"], a["pe"], a["ppe"], init_latents=a["z0"][:, :2], **s_kw)
    # the C entry point refuses the same combinations itself
    args, keep, mem, lat = eng._args(a["eps"], a["pe"], a["ppe"], a["cond"], a["pair"], 1.0)
    sig = sd3.flow_match_sigmas(2)
    out = np.empty_like(a["eps"])
    lib, h = eng.base.lib, eng.base._h

    def call(args, **fields):
        loop = sd3.pd_sd3_loop_args()
        for k, v in fields.items():
            setattr(loop, k, v.ctypes.data if isinstance(v, np.ndarray) else v)
        if lib.pd_sd3_sample_ex(h, C.byref(args), C.byref(loop), sig.ctypes.data, 2, 1.0, None, out.ctypes.data):
            raise E.PdError(lib.pd_last_error().decode())
    with pytest.raises(E.PdError, match="mask needs init_latents"):
        call(args, mask=a["mask"])
    with pytest.raises(E.PdError, match="PD_XT_FROM_SEED"):
        call(args, init_latents=a["z0"], noise=a["eps"], flags=sd3.PD_XT_FROM_SEED)
    with pytest.raises(E.PdError, match="PD_XT_FROM_SEED"):
        call(args, init_latents=a["z0"], flags=sd3.PD_XT_FROM_SEED)         # args->latents is set
    with pytest.raises(E.PdError, match="PD_INIT_PURE_NOISE needs"):
        call(args, flags=sd3.PD_INIT_PURE_NOISE)
    with pytest.raises(E.PdError, match="unknown flags"):
        call(args, init_latents=a["z0"], flags=64)
    with pytest.raises(E.PdError, match="noise needs init_latents"):
        call(args, noise=a["eps"])
    args.latents = None
    with pytest.raises(E.PdError, match="noise is required"):
        call(args, init_latents=a["z0"])
    # ... and an empty loop struct is the plain call
    args.latents = a["eps"].ctypes.data
    call(args)
    assert np.array_equal(out, eng.sample(a["eps"], a["pe"], a["ppe"], **s_kw))
    # PD_INIT_PURE_NOISE: the loop starts from eps whatever sigma_0 is (here 1, so it is the img2img result too)
    call(args, init_latents=a["z0"], mask=a["mask"], flags=sd3.PD_INIT_PURE_NOISE)
    assert np.array_equal(out, eng.sample(a["eps"], a["pe"], a["ppe"], init_latents=a["z0"], mask=a["mask"], **s_kw))


@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_two_byte_modes(sd, prec):
    """The plain loop (code this feature does not touch) is measured against the oracle first; the edited loops, at the same shape and
    precision against the restated loop, get twice that error.  Measured on one MI355X: see DESIGN.md, "SD3 img2img and inpainting"."""
    a = arrays(1, 8, 8, 6, 8)
    e = sd3.SD3Engine(CFG, precision=prec)
    try:
        e.load_state_dict(sd)
        kw = pipe_kw(a, latents=a["eps"])
        plain = Pipe(e)(**kw)["images"]
        base = relerr(plain, O.sample(sd, CFG, a["eps"], a["pe"], a["npe"], a["ppe"], a["nppe"], a["cond"], a["pair"], STEPS, GUIDE))
        img = relerr(Img2Img(e)(image=a["z0"], strength=0.5, **kw)["images"], ref_loop(sd, a, 0.5))
        out = Inpaint(e)(image=a["z0"], mask_image=a["mask_px"], strength=1.0, **kw)["images"]
        inp = relerr(out, ref_loop(sd, a, 1.0, a["mask"]))
        print(f"[sd3_edit] {prec}: plain loop {base:.3e}, img2img(0.5) {img:.3e}, inpaint(1.0) {inp:.3e} (allowed {2 * base:.3e})")
        assert 0.0 < base and img < 2 * base and inp < 2 * base
        keep = np.broadcast_to(a["mask"] == 0.0, out.shape)
        assert np.array_equal(out[keep], a["z0"][keep])
    finally:
        e.close()
