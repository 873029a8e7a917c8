"""The fused linear multistep loop (pd_lms_sample / pd_sample_begin_lms: PLMS and DPM-Solver++ multistep inside the engine)
on the GPU: against the host plug-in schedulers driving the same engine one eps evaluation at a time, and against the
trajectories the reference's own PLMSSampler / DPM_Solver produced on the TINY networks (tests/golden/samplers_lms.npz).

Bounds: fused against host plug-in per step 1e-5, the bound tests/test_unipc_fused_gpu.py uses for the same comparison;
against the reference trajectories 2e-4, the bound tests/test_network_gpu.py applies to the DDIM trajectory of the same
networks in f32 mode (the network error dominates and is characterised there)."""
import os

import numpy as np
import pytest

from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import weights as W
from prompt_diffusion_amd.pipeline import PromptDiffusionInpaintPipeline, PromptDiffusionPipeline
from prompt_diffusion_amd.schedulers import DPMSolverMultistepScheduler, PNDMScheduler
from tests import inpaint_ref as IR

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
FUSED_VS_HOST = 1e-5     # tests/test_unipc_fused_gpu.py
REFERENCE_TRAJ = 2e-4    # tests/test_network_gpu.py, TINY f32 DDIM trajectory


def relerr(a, b):
    return float(np.abs(np.asarray(a) - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module", params=["f32", "f16"])
def eng(request):
    e = E.Engine(W.TINY, precision=request.param)
    e.load_state_dict(W.synth_state_dict(W.TINY))
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng32():
    e = E.Engine(W.TINY, precision="f32")
    e.load_state_dict(W.synth_state_dict(W.TINY))
    yield e
    e.close()


def inputs(B=1, h=8, w=8, seed=21):
    inp = W.synth_inputs(W.TINY, B, h, w, seed=seed)
    return dict(x_T=inp["x_T"], ctx_cond=inp["ctx_cond"], ctx_uncond=inp["ctx_uncond"], pair=inp["pair"], query=inp["query"])


def host_loop(eng, sched, args, blend=None, replace=None):
    """The host plug-in driving the engine through pd_sample_eps_at: the sample after every completed step.
    blend: dict(ac, z0, eps, mask, grid) -- the inpainting blend in NumPy after every completed step.
    replace: (k, fn) -- after evaluation k the latents become fn(latents), as a callback that replaces them does."""
    a = dict(args)
    a.pop("timesteps", None)
    eng.sample_begin(steps=5, eta=0.0, **a)
    x = np.asarray(eng.sample_get(E.PD_GET_LATENTS))
    out, done = [], 0
    for i, t in enumerate(sched.timesteps):
        ends = sched.completes_step() if hasattr(sched, "completes_step") else True
        eps = np.asarray(eng.sample_eps_at(int(t)))
        x = sched.step(eps, t, x, return_dict=False)[0].astype(np.float32)
        if ends:
            if blend is not None:
                known = IR.known_after_step(blend["ac"], blend["z0"], blend["eps"], blend["grid"], done)
                x = IR.blend(known, x, blend["mask"]).astype(np.float32)
            done += 1
            out.append(x)
        if replace is not None and i == replace[0]:
            x = replace[1](x)
        eng.sample_set_latents(x)
    eng.sample_end()
    return out


SCHEDS = [("plms", lambda: PNDMScheduler())] + \
         [(f"dpmpp{o}", (lambda o=o: DPMSolverMultistepScheduler(solver_order=o))) for o in (1, 2, 3)]


@pytest.mark.parametrize("name,mk", SCHEDS)
@pytest.mark.parametrize("use_cfg", [True, False])
def test_fused_matches_host_plugin_per_step(eng, name, mk, use_cfg):
    sched = mk()
    sched.set_timesteps(6)
    args = dict(inputs(B=2), cfg_scale=4.0 if use_cfg else 1.0, use_cfg=use_cfg)
    host = host_loop(eng, sched, args)
    out, inter = eng.lms_sample(return_intermediates=True, **args, **sched.fused_lms())
    assert inter.shape[0] == 7 and len(host) == 6          # S + 1 entries, although PLMS runs S + 1 rows
    np.testing.assert_array_equal(inter[0], args["x_T"])
    np.testing.assert_array_equal(inter[-1], out)
    errs = [relerr(inter[i + 1], host[i]) for i in range(6)]
    print(f"[lms fused vs host] {name} cfg={use_cfg}: per-step relerr {['%.2e' % e for e in errs]}")
    assert max(errs) <= FUSED_VS_HOST


def _golden_args(fx):
    B, h, w = (int(v) for v in fx["tiny_shape"])
    inp = W.synth_inputs(W.TINY, B, h, w)
    return dict(x_T=inp["x_T"], ctx_cond=inp["ctx_cond"], ctx_uncond=inp["ctx_uncond"], pair=inp["pair"], query=inp["query"],
                use_cfg=False, cfg_scale=1.0)


def test_fused_plms_against_reference_trajectory(eng32):
    fx = np.load(os.path.join(GOLD, "samplers_lms.npz"))
    out, inter = eng32.lms_sample(return_intermediates=True, kind="plms", timesteps=fx["tiny_plms_s5_grid"], **_golden_args(fx))
    ref = fx["tiny_plms_s5_x"]
    errs = [relerr(inter[i], ref[i]) for i in range(len(ref))]
    print(f"[lms fused vs reference] plms: per-step relerr {['%.2e' % e for e in errs]}")
    assert max(errs) < REFERENCE_TRAJ


@pytest.mark.parametrize("tag", ["tiny_dpmpp_int_s9", "tiny_dpmpp_frac_s5"])
def test_fused_dpmpp_against_reference_trajectory(eng32, tag):
    fx = np.load(os.path.join(GOLD, "samplers_lms.npz"))
    mt = fx[tag + "_model_times"]
    out, inter = eng32.lms_sample(return_intermediates=True, kind="dpmsolver++", order=2, solver_type="dpm_solver",
                                  lower_order_final=True, model_times=mt, **_golden_args(fx))
    ref = fx[tag + "_x"]
    errs = [relerr(inter[i], ref[i]) for i in range(len(ref))]
    print(f"[lms fused vs reference] {tag}: per-step relerr {['%.2e' % e for e in errs]}")
    assert max(errs) < REFERENCE_TRAJ


@pytest.mark.parametrize("kw", [dict(kind="plms"), dict(kind="dpmsolver++", order=3)])
def test_graph_capture_and_replay_identical(eng32, kw):
    args = dict(inputs(seed=9), cfg_scale=3.0, timesteps=[999, 800, 600, 400, 200, 50])
    ref = eng32.lms_sample(**args, **kw)
    try:
        eng32.set_option("graph", 1)
        g1 = eng32.lms_sample(**args, **kw)      # captured
        g2 = eng32.lms_sample(**args, **kw)      # replayed
        ddim = eng32.ddim_sample(steps=6, **args)
        g3 = eng32.lms_sample(**args, **kw)      # the DDIM graph over the same grid and buffers is another one
    finally:
        eng32.set_option("graph", 0)
    for g in (g1, g2, g3):
        np.testing.assert_array_equal(g, ref)
    assert not np.array_equal(ddim, ref)


@pytest.mark.parametrize("name,mk,k", [("plms", SCHEDS[0][1], 0), ("plms", SCHEDS[0][1], 3), ("dpmpp2", SCHEDS[2][1], 2),
                                       ("dpmpp3", SCHEDS[3][1], 3)])
def test_stepwise_set_latents_midway_equals_host_with_same_replacement(eng32, name, mk, k):
    """pd_sample_set_latents after row k of the stepwise form against an independent result: the host plug-in loop given the
    same replacement at the same point.  The replacement depends on the current latents and changes them (it is no no-op);
    the solver's history and kept sample must survive it exactly as the host scheduler's do.  PLMS k = 0 replaces the trial
    sample between the two evaluations of the first step, which is redone from the kept sample."""
    def swap(x):
        return (np.float32(0.9) * np.asarray(x) + np.float32(0.05)).astype(np.float32)
    sched = mk()
    sched.set_timesteps(6)
    args = dict(inputs(B=2, seed=4), cfg_scale=3.0)
    host = host_loop(eng32, sched, args, replace=(k, swap))
    untouched = host_loop(eng32, (lambda s: (s.set_timesteps(6), s)[1])(mk()), args)
    fk = sched.fused_lms()
    rows, _ = eng32.lms_coefficients(fk.get("timesteps"), **{a: b for a, b in fk.items() if a != "timesteps"})
    n = eng32.sample_begin_lms(**args, **fk)
    assert n == len(rows) == len(sched.timesteps)
    fused = []
    for i in range(n):
        eng32.sample_step(i)
        if int(rows[i, 2]) & E.PD_LMS_F_STEP:
            fused.append(np.asarray(eng32.sample_get(E.PD_GET_LATENTS)))
        if i == k:
            eng32.sample_set_latents(swap(eng32.sample_get(E.PD_GET_LATENTS)))
    eng32.sample_end()
    assert len(fused) == len(host) == 6
    errs = [relerr(f, h) for f, h in zip(fused, host)]
    print(f"[lms set_latents after row {k}] {name}: per-step relerr {['%.2e' % e for e in errs]}")
    assert max(errs) <= FUSED_VS_HOST
    assert relerr(host[-1], untouched[-1]) > 1e-3      # the replacement did change the run


@pytest.mark.parametrize("name,mk", [SCHEDS[0], SCHEDS[2]])
def test_inpainting_equals_host_blend_and_all_ones_mask_is_plain(eng32, name, mk):
    sched = mk()
    sched.set_timesteps(5)
    base = dict(inputs(B=2, seed=6), cfg_scale=3.0)
    fk = sched.fused_lms()
    grid = fk["timesteps"]
    g = np.random.default_rng(2)
    z0 = g.standard_normal(base["x_T"].shape).astype(np.float32)
    mask = (g.random((2, 1, 8, 8)) > 0.5).astype(np.float32)
    fused, inter = eng32.lms_sample(return_intermediates=True, init_latents=z0, mask=mask, **base, **fk)
    ac = IR.alphas_cumprod_f32(W.TINY)
    start = IR.add_noise(ac, z0, base["x_T"], grid[0]).astype(np.float32)
    np.testing.assert_array_equal(inter[0], start)
    host = host_loop(eng32, sched, dict(base, x_T=start), blend=dict(ac=ac, z0=z0, eps=base["x_T"], mask=mask, grid=grid))
    errs = [relerr(inter[i + 1], host[i]) for i in range(5)]
    print(f"[lms inpaint fused vs host] {name}: per-step relerr {['%.2e' % e for e in errs]}")
    assert max(errs) <= FUSED_VS_HOST
    # an all-ones mask repaints everything: the img2img run without a mask, bit for bit
    ones = eng32.lms_sample(init_latents=z0, mask=np.ones_like(mask), **base, **fk)
    plain = eng32.lms_sample(init_latents=z0, **base, **fk)
    np.testing.assert_array_equal(ones, plain)


def test_one_update_launch_per_evaluation(eng32):
    """DDIM and the linear multistep loop end every evaluation with one update launch: the launch counter per evaluation is
    the same on the same grid."""
    args = dict(inputs(seed=3), cfg_scale=3.0, timesteps=[999, 800, 600, 400, 200, 50])

    def per_eval(begin, **kw):
        n = begin(**args, **kw)
        counts = []
        for i in range(n):
            l0 = eng32.stat("launches")
            eng32.sample_step(i)
            counts.append(eng32.stat("launches") - l0)
        eng32.sample_end()
        return counts
    ddim = per_eval(eng32.sample_begin, steps=6)
    assert len(set(ddim)) == 1
    for kw in (dict(kind="plms"), dict(kind="dpmsolver++", order=3)):
        got = per_eval(eng32.sample_begin_lms, **kw)
        assert set(got) == set(ddim), (kw, got, ddim)


def call_kw(B=2, hw=64, seed=21, **over):
    inp = W.synth_inputs(W.TINY, B, hw // 8, hw // 8, seed=seed, unit_range=True)
    a, b = inp["pair"][:, :3], inp["pair"][:, 3:]
    kw = dict(prompt_embeds=inp["ctx_cond"], negative_prompt_embeds=inp["ctx_uncond"], image=inp["query"].transpose(0, 2, 3, 1),
              image_pair=[a.transpose(0, 2, 3, 1), b.transpose(0, 2, 3, 1)], guidance_scale=4.0, latents=inp["x_T"],
              output_type="latent", num_inference_steps=6)
    kw.update(over)
    return kw


@pytest.mark.parametrize("mk", [lambda: DPMSolverMultistepScheduler(), lambda: PNDMScheduler()])
def test_pipeline_fused_agrees_with_host(eng32, mk):
    kw = call_kw()
    host = np.asarray(PromptDiffusionPipeline(eng32, scheduler=mk(), fuse_scheduler=False)(**kw).images)
    fused = np.asarray(PromptDiffusionPipeline(eng32, scheduler=mk(), fuse_scheduler=True)(**kw).images)
    seen = []
    step = np.asarray(PromptDiffusionPipeline(eng32, scheduler=mk(), fuse_scheduler=True)(
        callback_on_step_end=lambda p, i, t, k: seen.append(int(t)) or {}, **kw).images)
    err = relerr(fused, host)
    print(f"[lms pipeline fused vs host] {type(mk()).__name__}: relerr {err:.3e}")
    assert err <= FUSED_VS_HOST
    np.testing.assert_array_equal(step, fused)
    s = mk()
    s.set_timesteps(6)
    assert seen == [int(t) for t in s.timesteps]
    with pytest.raises(ValueError):
        PromptDiffusionPipeline(eng32, scheduler=object(), fuse_scheduler=True)


def test_sampler_facades_return_reference_shapes_and_keys(eng32):
    from prompt_diffusion_amd.ddim import ControlLDM, DPMSolverSampler, PLMSSampler
    fx = np.load(os.path.join(GOLD, "samplers_lms.npz"))
    B, h, w = (int(v) for v in fx["tiny_shape"])
    inp = W.synth_inputs(W.TINY, B, h, w)
    cond = {"c_crossattn": [inp["ctx_cond"]], "example_pair": [inp["pair"]], "query": [inp["query"]]}
    model = ControlLDM(eng32)
    samples, inter = PLMSSampler(model).sample(5, B, (4, h, w), cond, x_T=inp["x_T"], log_every_t=1, verbose=False)
    assert set(inter) == {"x_inter", "pred_x0"} and len(inter["x_inter"]) == len(inter["pred_x0"]) == 6
    assert np.asarray(samples).shape == (B, 4, h, w)
    # S = 5 on the reference's own grid: the fixture's trajectory, states and pred_x0
    errs = [relerr(inter["x_inter"][i], fx["tiny_plms_s5_x"][i]) for i in range(6)]
    errs += [relerr(inter["pred_x0"][i + 1], fx["tiny_plms_s5_pred_x0"][i]) for i in range(5)]
    assert max(errs) < REFERENCE_TRAJ
    with pytest.raises(ValueError):
        PLMSSampler(model).sample(5, B, (4, h, w), cond, x_T=inp["x_T"], eta=0.5, verbose=False)
    with pytest.raises(NotImplementedError):
        PLMSSampler(model).sample(5, B, (4, h, w), cond, x_T=inp["x_T"], quantize_x0=True, verbose=False)
    out, none = DPMSolverSampler(model).sample(5, B, (4, h, w), cond, x_T=inp["x_T"])
    assert none is None and np.asarray(out).shape == (B, 4, h, w)
    assert relerr(out, fx["tiny_dpmpp_frac_s5_x"][-1]) < REFERENCE_TRAJ


def test_engine_argument_errors(eng32):
    """A linear multistep solver draws no noise: eta != 0 or a noise tensor is refused, as is a grid that does not descend,
    an order outside 1..3 and img2img on fractional model times; the engine stays usable."""
    base = dict(inputs(seed=8), cfg_scale=3.0)
    ts = [801, 601, 401, 201, 1]
    noise = np.zeros((5,) + base["x_T"].shape, np.float32)
    with pytest.raises(E.PdError, match="eta must be 0"):
        eng32.lms_sample(kind="plms", timesteps=ts, eta=0.5, noise=noise, **base)
    with pytest.raises(E.PdError, match="eta must be 0"):
        eng32.lms_sample(kind="dpmsolver++", timesteps=ts, noise=noise, **base)
    with pytest.raises(E.PdError, match="descending"):
        eng32.lms_sample(kind="plms", timesteps=ts[::-1], **base)
    with pytest.raises(E.PdError, match="order"):
        eng32.lms_sample(kind="dpmsolver++", order=4, timesteps=ts, **base)
    with pytest.raises(E.PdError, match="integer grid"):
        eng32.lms_sample(kind="dpmsolver++", model_times=[999.0, 500.5, 0.0], init_latents=base["x_T"], **base)
    assert np.isfinite(eng32.lms_sample(kind="plms", timesteps=ts, **base)).all()


def inpaint_kw(B=2, hw=64, seed=13, **over):
    inp = W.synth_inputs(W.TINY, B, hw // 8, hw // 8, seed=seed, unit_range=True)
    a, b = inp["pair"][:, :3], inp["pair"][:, 3:]
    z0 = np.random.default_rng(seed).standard_normal((B, 4, hw // 8, hw // 8)).astype(np.float32)
    m = np.zeros((hw, hw), np.float32)
    m[:, hw // 2:] = 1.0
    kw = dict(prompt_embeds=inp["ctx_cond"], negative_prompt_embeds=inp["ctx_uncond"], control_image=inp["query"].transpose(0, 2, 3, 1),
              image_pair=[a.transpose(0, 2, 3, 1), b.transpose(0, 2, 3, 1)], guidance_scale=4.0, output_type="latent",
              image=z0, mask_image=m, num_inference_steps=10, controlnet_conditioning_scale=0.9)
    kw.update(over)
    return kw


@pytest.mark.parametrize("mk", [lambda: PNDMScheduler(), lambda: DPMSolverMultistepScheduler()])
@pytest.mark.parametrize("over", [dict(strength=1.0), dict(strength=0.8), dict(strength=0.9),
                                  dict(strength=0.6, control_guidance_start=0.15, control_guidance_end=0.7)])
def test_inpaint_pipeline_fused_agrees_with_host(eng32, mk, over):
    """PromptDiffusionInpaintPipeline with the new schedulers, fuse_scheduler on against off, after every evaluation: the
    host path takes its step count and blend levels from the scheduler's timesteps after set_begin_index and blends where a
    step completes, like the engine."""
    kw = inpaint_kw(**over)
    res = {}
    for fused in (False, True):
        pipe = PromptDiffusionInpaintPipeline(eng32, scheduler=mk(), fuse_scheduler=fused)
        seen = []
        out = np.asarray(pipe(callback_on_step_end=lambda p, i, t, k: seen.append((int(t), np.array(k["latents"]))) or {},
                              **dict(kw, generator=np.random.default_rng(2))).images)
        res[fused] = (out, seen)
        if fused:
            plain = np.asarray(pipe(**dict(kw, generator=np.random.default_rng(2))).images)
            np.testing.assert_array_equal(plain, out)
    (h, hs), (f, fs) = res[False], res[True]
    assert [t for t, _ in hs] == [t for t, _ in fs] and len(hs) >= 6
    errs = [relerr(a[1], b[1]) for a, b in zip(fs, hs)]
    print(f"[lms inpaint pipeline fused vs host] {type(mk()).__name__} {over}: {len(hs)} evaluations, max relerr {max(errs):.3e}")
    assert max(errs) <= FUSED_VS_HOST and relerr(f, h) <= FUSED_VS_HOST
    # the kept half of the image is the init latents themselves after the last step
    z0, half = kw["image"], kw["image"].shape[-1] // 2
    np.testing.assert_array_equal(f[..., :half], z0[..., :half])


def test_fractional_grid_takes_per_step_control_scales(eng32):
    """control_scales_step on a fractional grid is sized by the grid (5 steps here), not by a DDIM step count."""
    fx = np.load(os.path.join(GOLD, "samplers_lms.npz"))
    mt = fx["tiny_dpmpp_frac_s5_model_times"]
    args = _golden_args(fx)
    ones = eng32.lms_sample(model_times=mt, control_scales_step=np.ones((5, 13), np.float32), **args)
    np.testing.assert_array_equal(ones, eng32.lms_sample(model_times=mt, **args))
    half = eng32.lms_sample(model_times=mt, control_scales_step=np.full((5, 13), 0.5, np.float32), **args)
    assert not np.array_equal(half, ones)
    with pytest.raises(E.PdError, match="control_scales_step"):
        eng32.lms_sample(model_times=mt, control_scales_step=np.ones((6, 13), np.float32), **args)
