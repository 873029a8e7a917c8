"""img2img / inpainting inside the engine's loop (pd_sample_args.init_latents / mask / init_flags, sampler_update.hip) and the
PromptDiffusionImg2ImgPipeline / PromptDiffusionInpaintPipeline on the GPU: the fused loops against the stepwise loop with
the blend done in NumPy (bit-identical for DDIM), against the host UniPC scheduler, and against tests/inpaint_ref.py."""
import dataclasses

import numpy as np
import pytest

from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import weights as W
from prompt_diffusion_amd.pipeline import PromptDiffusionImg2ImgPipeline, PromptDiffusionInpaintPipeline
from prompt_diffusion_amd.schedulers import UniPCMultistepScheduler
from tests import inpaint_ref as R

pytestmark = pytest.mark.gpu

AC = R.alphas_cumprod_f32(W.TINY)
TS = [801, 601, 401, 201, 1]
LDM10 = list(range(901, 0, -100))   # the engine's 10-step DDIM grid, sampling order


def relerr(a, b):
    return float(np.abs(np.asarray(a) - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(W.TINY, precision="f32")
    e.load_state_dict(W.synth_state_dict(W.TINY))
    yield e
    e.close()


def case(B=2, hw=64, seed=7):
    inp = W.synth_inputs(W.TINY, B, hw // 8, hw // 8, seed=seed, unit_range=True)
    rng = np.random.default_rng(seed)
    z0 = rng.standard_normal(inp["x_T"].shape).astype(np.float32)
    mask = np.zeros((B, 1, hw // 8, hw // 8), np.float32)
    mask[:, :, :, hw // 16:] = 1.0
    mask[-1, :, : hw // 16] = 1.0
    args = dict(x_T=inp["x_T"], ctx_cond=inp["ctx_cond"], ctx_uncond=inp["ctx_uncond"], pair=inp["pair"], query=inp["query"],
                steps=len(TS), cfg_scale=4.0, timesteps=TS)
    return args, z0, mask


def stepwise(eng, args, z0, mask, pure=False):
    """the plain stepwise loop from the NumPy start, the blend in NumPy between steps (sample_get / sample_set_latents)"""
    eps, ts = args["x_T"], args["timesteps"]
    x = R.start_latents(AC, z0, eps, ts, True, 1.0 if pure else 0.5)
    eng.sample_begin(**dict(args, x_T=x))
    out = [x]
    try:
        for i in range(len(ts)):
            eng.sample_step(i)
            x = eng.sample_get()
            if mask is not None:
                x = R.blend(R.known_after_step(AC, z0, eps, ts, i), x, mask)
                eng.sample_set_latents(x)
            out.append(x)
    finally:
        eng.sample_end()
    return np.stack(out)


@pytest.mark.parametrize("over", [dict(), dict(use_cfg=False, cfg_scale=1.0), dict(guess_mode=True), dict(eta=0.5)])
def test_fused_ddim_inpaint_bit_identical_to_stepwise(eng, over):
    args, z0, mask = case()
    args.update(over)
    if over.get("eta"):
        args["noise"] = np.random.default_rng(1).standard_normal((len(TS),) + z0.shape).astype(np.float32)
    for pure in (False, True):
        ref = stepwise(eng, args, z0, mask, pure)
        lat, inter = eng.ddim_sample(init_latents=z0, mask=mask, init_pure_noise=pure, return_intermediates=True, **args)
        for i in range(len(TS) + 1):
            np.testing.assert_array_equal(inter[i], ref[i], err_msg=f"step {i} pure {pure}")
        np.testing.assert_array_equal(lat, ref[-1])
        keep = mask.repeat(4, 1) == 0     # the kept region is z0 exactly after the last step
        np.testing.assert_array_equal(lat[keep], z0[keep])


def test_img2img_start_and_plain_equivalence(eng):
    args, z0, _ = case(seed=3)
    lat, inter = eng.ddim_sample(init_latents=z0, return_intermediates=True, **args)
    start = R.add_noise(AC, z0, args["x_T"], TS[0])
    np.testing.assert_array_equal(inter[0], start)
    np.testing.assert_array_equal(lat, eng.ddim_sample(**dict(args, x_T=start)))
    # invariants: an all-ones mask is img2img without a mask, an all-zeros mask returns z0
    ones = np.ones((1, 1) + z0.shape[2:], np.float32)      # [1, 1, h, w] broadcasts over the batch
    np.testing.assert_array_equal(eng.ddim_sample(init_latents=z0, mask=ones, **args), lat)
    np.testing.assert_array_equal(eng.ddim_sample(init_latents=z0, mask=0 * ones, **args), z0)


def test_device_tensors(eng):
    import torch
    args, z0, mask = case(seed=5)
    ref = eng.ddim_sample(init_latents=z0, mask=mask, **args)
    d = {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in args.items()}
    got = eng.ddim_sample(init_latents=torch.from_numpy(z0).cuda(), mask=torch.from_numpy(mask[:1]).cuda(), **d)
    ref1 = eng.ddim_sample(init_latents=z0, mask=np.repeat(mask[:1], 2, 0), **args)
    np.testing.assert_array_equal(got.cpu().numpy(), ref1)
    assert not np.array_equal(ref1, ref)


def test_graph_replay_and_key(eng):
    args, z0, mask = case(B=1, seed=9)
    plain = eng.ddim_sample(**args)
    inp = eng.ddim_sample(init_latents=z0, mask=mask, **args)
    i2i = eng.ddim_sample(init_latents=z0, **args)
    pure = eng.ddim_sample(init_latents=z0, mask=mask, init_pure_noise=True, **args)
    uni = eng.unipc_sample(init_latents=z0, mask=mask, **args)
    try:
        eng.set_option("graph", 1)
        for _ in range(2):   # captured, then replayed; a plain call never replays an inpainting graph, nor the reverse
            np.testing.assert_array_equal(eng.ddim_sample(**args), plain)
            np.testing.assert_array_equal(eng.ddim_sample(init_latents=z0, mask=mask, **args), inp)
            np.testing.assert_array_equal(eng.ddim_sample(**args), plain)
            np.testing.assert_array_equal(eng.ddim_sample(init_latents=z0, **args), i2i)
            np.testing.assert_array_equal(eng.ddim_sample(init_latents=z0, mask=mask, init_pure_noise=True, **args), pure)
            np.testing.assert_array_equal(eng.unipc_sample(init_latents=z0, mask=mask, **args), uni)
    finally:
        eng.set_option("graph", 0)
    assert not np.array_equal(inp, plain) and not np.array_equal(inp, pure) and not np.array_equal(i2i, inp)


def test_launches_per_step(eng):
    args, z0, mask = case(B=1, seed=2)

    def per_step(begin, **kw):
        n = begin(**kw)
        try:
            c0 = eng.stat("launches")
            for i in range(n):
                eng.sample_step(i)
            return (eng.stat("launches") - c0) / n
        finally:
            eng.sample_end()

    plain = per_step(eng.sample_begin, **args)
    assert per_step(eng.sample_begin, init_latents=z0, mask=mask, **args) == plain
    assert per_step(eng.sample_begin_unipc, init_latents=z0, mask=mask, **args) == per_step(eng.sample_begin_unipc, **args)


def test_stepwise_blend_survives_set_latents(eng):
    """pd_sample_step blends after a pd_sample_set_latents too; pd_sample_eps_at never updates or blends"""
    args, z0, mask = case(B=1, seed=4)
    eng.sample_begin(init_latents=z0, mask=mask, **args)
    try:
        eng.sample_step(0)
        x = eng.sample_get() * np.float32(0.5)
        eng.sample_set_latents(x)
        eng.sample_eps_at(TS[1])
        np.testing.assert_array_equal(eng.sample_get(), x)
        eng.sample_step(1)
        got = eng.sample_get()
    finally:
        eng.sample_end()
    eng.sample_begin(**dict(args, x_T=x))   # the plain loop from x at step 1, then the NumPy blend
    try:
        eng.sample_step(1)
        ref = R.blend(R.known_after_step(AC, z0, args["x_T"], TS, 1), eng.sample_get(), mask)
    finally:
        eng.sample_end()
    np.testing.assert_array_equal(got, ref)


def test_rejections(eng):
    args, z0, mask = case(B=1)
    with pytest.raises(E.PdError, match="mask needs init_latents"):
        eng.ddim_sample(mask=mask, **args)
    with pytest.raises(E.PdError, match="PD_INIT_PURE_NOISE needs init_latents"):
        eng.ddim_sample(init_pure_noise=True, **args)
    a, keep, _ = eng._args(init_latents=z0, **args)
    a.init_flags = 6
    out = np.empty_like(z0)
    assert eng.lib.pd_ddim_sample(eng._h, E.C.byref(a), 0, out.ctypes.data, None) != 0
    assert "init_flags" in eng.lib.pd_last_error().decode()
    del keep
    assert np.isfinite(eng.ddim_sample(init_latents=z0, mask=mask, **args)).all()


# ---------------------------------------------------------------------------------------------------------------- pipelines
def pipe_kw(B=1, hw=64, seed=11, **over):
    inp = W.synth_inputs(W.TINY, B, hw // 8, hw // 8, seed=seed, unit_range=True)
    a, b = inp["pair"][:, :3], inp["pair"][:, 3:]
    rng = np.random.default_rng(seed)
    z0 = rng.standard_normal((B, 4, hw // 8, hw // 8)).astype(np.float32)
    m = np.zeros((hw, hw), np.float32)
    m[:, hw // 2:] = 1.0
    kw = dict(prompt_embeds=inp["ctx_cond"], negative_prompt_embeds=inp["ctx_uncond"], control_image=inp["query"].transpose(0, 2, 3, 1),
              image_pair=[a.transpose(0, 2, 3, 1), b.transpose(0, 2, 3, 1)], guidance_scale=4.0, output_type="latent",
              image=z0, mask_image=m, num_inference_steps=10, controlnet_conditioning_scale=0.9)
    kw.update(over)
    return kw, inp, z0, m


def collect(pipe, kw):
    seen = []
    out = np.asarray(pipe(callback_on_step_end=lambda p, i, t, k: seen.append(np.array(k["latents"])) or {}, **kw).images)
    return out, seen


@pytest.mark.parametrize("strength", [1.0, 0.6])
def test_inpaint_pipeline_paths_agree_with_reference(eng, strength):
    kw, inp, z0, m = pipe_kw(B=2, strength=strength, generator=np.random.default_rng(5), control_guidance_end=0.7)
    fused = np.asarray(PromptDiffusionInpaintPipeline(eng)(**kw).images)
    kw["generator"] = np.random.default_rng(5)
    cb, seen = collect(PromptDiffusionInpaintPipeline(eng), kw)
    np.testing.assert_array_equal(cb, fused)
    # the restatement: the plain engine loop on the truncated grid, diffusers' start and blend in NumPy
    eps = np.random.default_rng(5).standard_normal(z0.shape, dtype=np.float32)
    ts, _ = R.get_timesteps(LDM10, strength)
    mask = R.process_mask(m[None, None], 2)
    keep = [1.0 - float((i + 1) / len(ts) > 0.7) for i in range(len(ts))]
    x0 = R.start_latents(AC, z0, eps, ts, True, strength)
    eng.sample_begin(x_T=x0, ctx_cond=inp["ctx_cond"], ctx_uncond=inp["ctx_uncond"], pair=inp["pair"],
                     query=inp["query"], steps=len(ts), cfg_scale=4.0, timesteps=ts,
                     control_scales_step=np.stack([np.full(13, 0.9 * k, np.float32) for k in keep]))

    def step(i, x):
        eng.sample_set_latents(x)
        eng.sample_step(i)
        return eng.sample_get()

    try:
        ref = R.run_loop(step, AC, z0, eps, mask, ts, x0)
    finally:
        eng.sample_end()
    assert len(seen) == len(ref) == len(ts)
    for i, (s, r) in enumerate(zip(seen, ref)):
        np.testing.assert_array_equal(s, r, err_msg=f"step {i}")


@pytest.mark.parametrize("strength", [1.0, 0.7])
def test_unipc_fused_and_host_agree(eng, strength):
    kw, _, _, _ = pipe_kw(B=2, seed=13, strength=strength)
    res = {}
    for fused in (False, True):
        sched = UniPCMultistepScheduler(solver_order=2, disable_corrector=[4])
        pipe = PromptDiffusionInpaintPipeline(eng, scheduler=sched, fuse_scheduler=fused)
        res[fused] = collect(pipe, dict(kw, generator=np.random.default_rng(2)))
        if fused:
            plain = np.asarray(pipe(**dict(kw, generator=np.random.default_rng(2))).images)
            np.testing.assert_array_equal(plain, res[True][0])
    (h, hs), (f, fs) = res[False], res[True]
    assert len(hs) == len(fs) == int(10 * strength)
    errs = [relerr(a, b) for a, b in zip(fs, hs)]
    print(f"[inpaint unipc fused vs host] strength {strength}: max per-step relerr {max(errs):.3e}")
    assert max(errs) <= 1e-5


def test_img2img_pipeline(eng):
    kw, inp, z0, _ = pipe_kw(B=1, seed=17)
    kw.pop("mask_image")
    eps = np.random.default_rng(8).standard_normal(z0.shape, dtype=np.float32)
    pipe = PromptDiffusionImg2ImgPipeline(eng)
    base = dict(ctx_cond=inp["ctx_cond"], ctx_uncond=inp["ctx_uncond"], pair=inp["pair"], query=inp["query"], cfg_scale=4.0,
                control_scales=[0.9] * 13)
    out = np.asarray(pipe(**dict(kw, strength=0.6, latents=eps)).images)
    ts, _ = R.get_timesteps(LDM10, 0.6)
    ref = eng.ddim_sample(x_T=R.add_noise(AC, z0, eps, ts[0]), steps=len(ts), timesteps=ts, **base)
    np.testing.assert_array_equal(out, ref)
    # strength 1 still starts from add_noise at the first timestep; the callback path is the same computation
    out1 = np.asarray(pipe(**dict(kw, strength=1.0, latents=eps)).images)
    cb1, _ = collect(pipe, dict(kw, strength=1.0, latents=eps))
    np.testing.assert_array_equal(cb1, out1)
    np.testing.assert_array_equal(out1, eng.ddim_sample(x_T=R.add_noise(AC, z0, eps, 901), steps=10, **base))
    # num_images_per_prompt: the init latents are repeated to the batch
    many = np.asarray(pipe(**dict(kw, strength=0.6, num_images_per_prompt=2, latents=np.concatenate([eps, eps]))).images)
    np.testing.assert_array_equal(many[0], many[1])
    assert relerr(many[0], out[0]) <= 1e-5


def test_f16_engine():
    e = E.Engine(W.TINY, precision="f16")
    try:
        e.load_state_dict(W.synth_state_dict(W.TINY))
        args, z0, mask = case(seed=19)
        for pure in (False, True):
            ref = stepwise(e, args, z0, mask, pure)
            _, inter = e.ddim_sample(init_latents=z0, mask=mask, init_pure_noise=pure, return_intermediates=True, **args)
            np.testing.assert_array_equal(inter, ref)
    finally:
        e.close()


def test_vae_encoded_init_image_and_draw_order():
    cfg = dataclasses.replace(W.TINY, vae_encoder=True)
    e = E.Engine(cfg, precision="f32")
    try:
        for n, a in W.synth_vae_encoder_state_dict(cfg).items():
            e.load_tensor(n, a)
        e.load_state_dict(W.synth_state_dict(cfg))
        kw, inp, _, m = pipe_kw(B=1, seed=23, strength=0.5)
        img = np.random.default_rng(3).uniform(0, 1, (1, 64, 64, 3)).astype(np.float32)
        out = np.asarray(PromptDiffusionInpaintPipeline(e)(**dict(kw, image=img, generator=np.random.default_rng(9))).images)
        # diffusers' order: the posterior draw first, then the noise draw from the same generator
        g = np.random.default_rng(9)
        post = g.standard_normal((1, 4, 8, 8), dtype=np.float32)
        z0 = e.vae_encode(np.ascontiguousarray(img.transpose(0, 3, 1, 2)) * np.float32(2) - np.float32(1), mode="sample", noise=post)
        ref = np.asarray(PromptDiffusionInpaintPipeline(e)(**dict(kw, image=z0, generator=g)).images)
        np.testing.assert_array_equal(out, ref)
        assert relerr(out, np.asarray(PromptDiffusionInpaintPipeline(e)(**dict(kw, image=z0, generator=np.random.default_rng(9))).images)) > 0
    finally:
        e.close()
