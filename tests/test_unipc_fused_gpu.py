"""The fused UniPC loop (pd_unipc_sample / pd_sample_begin_unipc, PromptDiffusionPipeline(fuse_scheduler=True)) on the GPU,
against the host plug-in UniPCMultistepScheduler driving the same engine one eps evaluation at a time, and against the
oracle network with the oracle's closed-form UniPC."""
import numpy as np
import pytest

from oracle import pd_oracle as O
from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import weights as W
from prompt_diffusion_amd.pipeline import PromptDiffusionPipeline
from prompt_diffusion_amd.schedulers import UniPCMultistepScheduler

pytestmark = pytest.mark.gpu


def relerr(a, b):
    return float(np.abs(np.asarray(a) - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(W.TINY, precision="f32")
    e.load_state_dict(W.synth_state_dict(W.TINY))
    yield e
    e.close()


def call_kw(B=1, hw=64, seed=21, **over):
    inp = W.synth_inputs(W.TINY, B, hw // 8, hw // 8, seed=seed, unit_range=True)
    a, b = inp["pair"][:, :3], inp["pair"][:, 3:]
    kw = dict(prompt_embeds=inp["ctx_cond"], negative_prompt_embeds=inp["ctx_uncond"], image=inp["query"].transpose(0, 2, 3, 1),
              image_pair=[a.transpose(0, 2, 3, 1), b.transpose(0, 2, 3, 1)], guidance_scale=4.0, latents=inp["x_T"],
              output_type="latent")
    kw.update(over)
    return kw, inp


def run(eng, fused, sched_kw, kw, cb=None):
    """final latents and the latents after every step (collected by a callback_on_step_end)"""
    pipe = PromptDiffusionPipeline(eng, scheduler=UniPCMultistepScheduler(**sched_kw), fuse_scheduler=fused)
    seen = []

    def collect(p, i, t, k):
        seen.append(np.array(k["latents"]))
        return cb(p, i, t, k) if cb is not None else {}

    out = np.asarray(pipe(callback_on_step_end=collect, **kw).images)
    return out, seen


@pytest.mark.parametrize("steps", [5, 20])
def test_fused_matches_host_scheduler_per_step(eng, steps):
    worst = 0.0
    kw, _ = call_kw(B=2, num_inference_steps=steps, controlnet_conditioning_scale=0.9)
    for order in (1, 2, 3):
        for st in ("bh1", "bh2"):
            sk = dict(solver_order=order, solver_type=st, disable_corrector=[1])
            host, hs = run(eng, False, sk, kw)
            fused, fs = run(eng, True, sk, kw)
            assert len(hs) == len(fs) == steps
            for i, (f, h) in enumerate(zip(fs, hs)):
                err = relerr(f, h)
                assert err <= 1e-5, (order, st, i, err)
                worst = max(worst, err)
            # the loop without callbacks (pd_unipc_sample) is the same computation
            pipe = PromptDiffusionPipeline(eng, scheduler=UniPCMultistepScheduler(**sk), fuse_scheduler=True)
            np.testing.assert_array_equal(np.asarray(pipe(**kw).images), fused)
    print(f"[unipc fused vs host] {steps} steps: max per-step relerr {worst:.3e}")


def test_fused_against_oracle_replay(eng):
    """test_pipeline_with_unipc_scheduler_against_oracle_replay's setup with the update inside the engine."""
    cfg = W.TINY
    B, hw, S, gs, scale, g_end = 1, 64, 5, 4.0, 0.9, 0.8
    inp = W.synth_inputs(cfg, B, hw // 8, hw // 8, seed=21, unit_range=True)
    sd = W.synth_state_dict(cfg)
    lay = O.make_layouts(cfg, W)
    sched = UniPCMultistepScheduler()
    pipe = PromptDiffusionPipeline(eng, scheduler=sched, fuse_scheduler=True)
    a, b = inp["pair"][:, :3], inp["pair"][:, 3:]
    out = pipe(prompt_embeds=inp["ctx_cond"], negative_prompt_embeds=inp["ctx_uncond"], image=inp["query"].transpose(0, 2, 3, 1),
               image_pair=[a.transpose(0, 2, 3, 1), b.transpose(0, 2, 3, 1)], num_inference_steps=S, guidance_scale=gs,
               latents=inp["x_T"], output_type="latent", controlnet_conditioning_scale=scale, control_guidance_end=g_end).images
    ts = [int(t) for t in sched.timesteps]
    keep = {t: 1.0 - float((i + 1) / S > g_end) for i, t in enumerate(ts)}
    pe, ne, pair, query = inp["ctx_cond"], inp["ctx_uncond"], inp["pair"], inp["query"]

    def eps_fn(x, t):
        x = x.astype(np.float32)
        x_in = np.concatenate([x, x]); t_in = np.full((2 * B,), t, np.int64)
        ctx = np.concatenate([ne, pe]); pr = np.concatenate([pair, pair]); qr = np.concatenate([query, query])
        ctl = [c * np.float32(scale * keep[t]) for c in O.controlnet_forward(sd, cfg, lay, x_in, t_in, pr, qr, ctx)]
        eps = O.controlled_unet_forward(sd, cfg, lay, x_in, t_in, ctx, ctl)
        return eps[:B] + np.float32(gs) * (eps[B:] - eps[:B])

    ref = O.unipc2_sample(eps_fn, inp["x_T"], sched.alphas_cumprod, ts)
    err = relerr(out, ref)
    print(f"[unipc fused vs oracle] relerr {err:.3e}")
    assert err < 5e-4


@pytest.mark.parametrize("over", [dict(guess_mode=True, controlnet_conditioning_scale=0.8),
                                  dict(control_guidance_start=0.2, control_guidance_end=0.6),
                                  dict(guidance_scale=1.0)])
def test_fused_matches_host_guess_window_no_cfg(eng, over):
    kw, _ = call_kw(B=2, seed=5, num_inference_steps=6, **over)
    host, hs = run(eng, False, {}, kw)
    fused, fs = run(eng, True, {}, kw)
    errs = [relerr(f, h) for f, h in zip(fs, hs)]
    print(f"[unipc fused vs host] {over}: max per-step relerr {max(errs):.3e}")
    assert max(errs) <= 1e-5


def test_graph_replay_and_key(eng):
    _, inp = call_kw(B=1, seed=9)
    args = dict(x_T=inp["x_T"], ctx_cond=inp["ctx_cond"], ctx_uncond=inp["ctx_uncond"], pair=inp["pair"], query=inp["query"],
                steps=6, cfg_scale=3.0, timesteps=[999, 800, 600, 400, 200, 50])   # order 3 reaches 3 at step 2
    ref = eng.unipc_sample(order=3, **args)
    try:
        eng.set_option("graph", 1)
        g1 = eng.unipc_sample(order=3, **args)      # captured
        g2 = eng.unipc_sample(order=3, **args)      # replayed
        ddim = eng.ddim_sample(**args)              # same shapes, grid and buffers: must not replay the UniPC graph
        g3 = eng.unipc_sample(order=3, **args)      # ... nor the DDIM graph
        o2 = eng.unipc_sample(order=2, **args)      # other coefficients, other graph
    finally:
        eng.set_option("graph", 0)
    np.testing.assert_array_equal(g1, ref)
    np.testing.assert_array_equal(g2, ref)
    np.testing.assert_array_equal(g3, ref)
    assert not np.array_equal(ddim, ref)
    np.testing.assert_array_equal(ddim, eng.ddim_sample(**args))
    np.testing.assert_array_equal(o2, eng.unipc_sample(order=2, **args))
    assert not np.array_equal(o2, ref)


def test_callbacks_and_getters(eng):
    kw, inp = call_kw(B=1, seed=13, num_inference_steps=6)
    pipe = PromptDiffusionPipeline(eng, scheduler=UniPCMultistepScheduler(), fuse_scheduler=True)
    plain = np.asarray(pipe(**kw).images)
    noop = np.asarray(pipe(callback_on_step_end=lambda p, i, t, k: {}, **kw).images)
    np.testing.assert_array_equal(noop, plain)
    legacy = []
    np.testing.assert_array_equal(np.asarray(pipe(callback=lambda i, t, lat: legacy.append(i), callback_steps=2, **kw).images), plain)
    assert legacy == [0, 2, 4]

    def scale(p, i, t, k):
        return {"latents": k["latents"] * np.float32(0.9)} if i == 2 else {}

    host, hs = run(eng, False, {}, kw, cb=scale)
    fused, fs = run(eng, True, {}, kw, cb=scale)
    err = max(relerr(f, h) for f, h in zip(fs, hs))
    assert err <= 1e-5
    assert relerr(fused, plain) > 1e-3          # the callback's latents were taken over
    # PD_GET_PRED_X0 is m_i = (x_i - sigma_i eps_i) / alpha_i, PD_GET_EPS the guided eps of the step
    ts = [999, 800, 500, 200]
    coef = E.unipc_coefficients(W.TINY, ts, order=2)
    eng.sample_begin_unipc(x_T=inp["x_T"], ctx_cond=inp["ctx_cond"], ctx_uncond=inp["ctx_uncond"], pair=inp["pair"],
                           query=inp["query"], steps=len(ts), cfg_scale=4.0, timesteps=ts)
    try:
        for i in range(len(ts)):
            x = eng.sample_get(E.PD_GET_LATENTS).astype(np.float64)
            eng.sample_step(i)
            e = eng.sample_get(E.PD_GET_EPS).astype(np.float64)
            m = eng.sample_get(E.PD_GET_PRED_X0)
            np.testing.assert_allclose(m, (x - coef[i, 1] * e) / coef[i, 0], rtol=1e-6, atol=1e-6 * np.abs(m).max())
    finally:
        eng.sample_end()


def test_f16_engine_against_host():
    e = E.Engine(W.TINY, precision="f16")
    try:
        e.load_state_dict(W.synth_state_dict(W.TINY))
        kw, _ = call_kw(B=2, seed=3, num_inference_steps=8)
        host, _ = run(e, False, dict(solver_order=3), kw)
        fused, _ = run(e, True, dict(solver_order=3), kw)
        err = relerr(fused, host)
        print(f"[unipc fused vs host] f16: relerr {err:.3e}")
        assert err <= 5e-3
    finally:
        e.close()


def test_rejections(eng):
    with pytest.raises(ValueError, match="alphas_cumprod"):
        PromptDiffusionPipeline(eng, scheduler=UniPCMultistepScheduler(beta_schedule="linear"), fuse_scheduler=True)
    with pytest.raises(ValueError, match="num_train_timesteps"):
        PromptDiffusionPipeline(eng, scheduler=UniPCMultistepScheduler(num_train_timesteps=500), fuse_scheduler=True)

    class Foreign:
        timesteps = np.zeros(0, np.int64)

    with pytest.raises(ValueError, match="UniPCMultistepScheduler"):
        PromptDiffusionPipeline(eng, scheduler=Foreign(), fuse_scheduler=True)
    with pytest.raises(ValueError, match="UniPCMultistepScheduler"):
        PromptDiffusionPipeline(eng, fuse_scheduler=True)
    _, inp = call_kw(B=1, seed=2)
    args = dict(x_T=inp["x_T"], ctx_cond=inp["ctx_cond"], ctx_uncond=inp["ctx_uncond"], pair=inp["pair"], query=inp["query"],
                steps=3, cfg_scale=3.0)
    ts = [900, 500, 100]
    with pytest.raises(E.PdError, match="eta"):
        eng.unipc_sample(eta=0.5, noise=np.zeros((3,) + inp["x_T"].shape, np.float32), timesteps=ts, **args)
    with pytest.raises(E.PdError, match="noise"):
        eng.unipc_sample(noise=np.zeros((3,) + inp["x_T"].shape, np.float32), timesteps=ts, **args)
    with pytest.raises(E.PdError, match="required"):
        eng.unipc_sample(**args)
    with pytest.raises(E.PdError, match="order"):
        eng.sample_begin_unipc(order=4, timesteps=ts, **args)
    with pytest.raises(E.PdError, match="strictly descending"):
        eng.unipc_sample(timesteps=[900, 500, 500], **args)
    # the engine is usable afterwards
    assert np.isfinite(eng.unipc_sample(timesteps=ts, **args)).all()
