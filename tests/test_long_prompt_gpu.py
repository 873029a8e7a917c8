"""Context lengths other than 77 end to end: pd_sample_args.context_len through every sampling entry point on the reduced network
(generic attention path) against the NumPy oracle, through the fused transformer tail on a one-level 320-channel network, and the
pipeline's long prompts (the reference's three 75-token windows, cldm/hack.py) on the engine's own CLIP.

Bounds: 2e-4 per step for the fp32 engine against the oracle's trajectory (tests/test_network_gpu.py, tests/test_lms_gpu.py:
REFERENCE_TRAJ); the f16 block bound of tests/test_st_tail_gpu.py (5e-3) per step for the fused tail against the per-layer path."""
import dataclasses
import os

import numpy as np
import pytest

from oracle import pd_oracle as O
from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import weights as W
from prompt_diffusion_amd.pipeline import PromptDiffusionPipeline
from prompt_diffusion_amd.schedulers import DPMSolverMultistepScheduler, UniPCMultistepScheduler
from tests.long_prompt_stub import TOKEN_COUNTS, StubTokenizer, prompt_of

pytestmark = pytest.mark.gpu
TRAJ = 2e-4
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def relerr(a, b):
    return float(np.abs(np.asarray(a) - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def net():
    return W.synth_state_dict(W.TINY), O.make_layouts(W.TINY, W)


@pytest.fixture(scope="module")
def eng(net):
    e = E.Engine(W.TINY, precision="f32")
    e.load_state_dict(net[0])
    yield e
    e.close()


def inputs(L, B=1, h=8, w=8, seed=31):
    inp = W.synth_inputs(W.TINY, B, h, w, seed=seed)
    r = np.random.default_rng(seed + 1000 * L)
    D = W.TINY.context_dim
    return dict(x_T=inp["x_T"], pair=inp["pair"], query=inp["query"],
                ctx_cond=r.standard_normal((B, L, D), dtype=np.float32), ctx_uncond=r.standard_normal((B, L, D), dtype=np.float32))


def oracle_eps(net, a, gs, guess=False, only_mid=False):
    """guided eps of the oracle's networks on the inputs `a` (uncond half first, ddim_hacked.py:188-193; guess mode as the (D) pipeline)"""
    sd, lay = net
    cfg, B = W.TINY, a["x_T"].shape[0]
    ctx = np.concatenate([a["ctx_uncond"], a["ctx_cond"]])
    pr, qr = np.concatenate([a["pair"]] * 2), np.concatenate([a["query"]] * 2)

    def fn(x, t):
        x = np.asarray(x, np.float32)
        x_in, t_in = np.concatenate([x, x]), np.full((2 * B,), int(t), np.int64)
        if guess:
            ctl = O.controlnet_forward(sd, cfg, lay, x, t_in[:B], a["pair"], a["query"], a["ctx_cond"])
            ctl = [np.concatenate([np.zeros_like(c), c]) for c in ctl]
        else:
            ctl = O.controlnet_forward(sd, cfg, lay, x_in, t_in, pr, qr, ctx)
        eps = O.controlled_unet_forward(sd, cfg, lay, x_in, t_in, ctx, ctl, only_mid)
        return eps[:B] + np.float32(gs) * (eps[B:] - eps[:B])
    return fn


def host_trajectory(sched, eps_fn, x_T):
    """a NumPy scheduler of this package driven by the oracle's eps: the sample after every step"""
    x, out = x_T, []
    for t in sched.timesteps:
        x = sched.step(eps_fn(x, int(t)), t, x, return_dict=False)[0].astype(np.float32)
        out.append(x)
    return out


@pytest.mark.parametrize("L", [231, 40])
def test_ddim_unipc_lms_match_the_oracle_trajectory(eng, net, L):
    sd, lay = net
    a = inputs(L)
    S, gs = 4, 5.0
    cond = dict(c_crossattn=a["ctx_cond"], example_pair=a["pair"], query=a["query"])
    unc = dict(c_crossattn=a["ctx_uncond"], example_pair=a["pair"], query=a["query"])
    # DDIM
    _, ref, _ = O.ddim_sampling(sd, W.TINY, lay, S, a["x_T"], cond, unc, gs)
    out, inter = eng.ddim_sample(steps=S, cfg_scale=gs, return_intermediates=True, **a)
    errs = [relerr(inter[i], ref[i]) for i in range(len(ref))]
    print(f"[L {L}] ddim per-step relerr {['%.2e' % v for v in errs]}")
    assert max(errs) < TRAJ
    fn = oracle_eps(net, a, gs)
    # UniPC (order 2, bh2)
    sched = UniPCMultistepScheduler()
    sched.set_timesteps(S)
    ref = host_trajectory(sched, fn, a["x_T"])
    out, inter = eng.unipc_sample(timesteps=[int(t) for t in sched.timesteps], order=sched.solver_order, solver_type=sched.solver_type,
                                  lower_order_final=sched.lower_order_final, cfg_scale=gs, steps=S, return_intermediates=True, **a)
    errs = [relerr(inter[i + 1], ref[i]) for i in range(S)]
    print(f"[L {L}] unipc per-step relerr {['%.2e' % v for v in errs]}")
    assert max(errs) < TRAJ
    # DPM-Solver++ 2M through the linear multistep loop
    sched = DPMSolverMultistepScheduler(solver_order=2)
    sched.set_timesteps(S)
    ref = host_trajectory(sched, fn, a["x_T"])
    out, inter = eng.lms_sample(cfg_scale=gs, return_intermediates=True, **a, **sched.fused_lms())
    errs = [relerr(inter[i + 1], ref[i]) for i in range(S)]
    print(f"[L {L}] dpm++ per-step relerr {['%.2e' % v for v in errs]}")
    assert max(errs) < TRAJ


def test_explicit_77_is_the_default_and_bad_lengths_are_refused(eng):
    import ctypes as C
    a = inputs(77, seed=33)
    ref = eng.ddim_sample(steps=2, cfg_scale=4.0, **a)
    args, keep, (B, h, w) = eng._args(steps=2, cfg_scale=4.0, **a)
    assert args.context_len == 77
    for L in (0, 77):
        args.context_len = L
        out = np.empty_like(ref)
        eng._check(eng.lib.pd_ddim_sample(eng._h, C.byref(args), args.mem, out.ctypes.data, None))
        np.testing.assert_array_equal(out, ref)
    for L in (-1, E.PD_MAX_CONTEXT_LEN + 1):
        args.context_len = L
        assert eng.lib.pd_ddim_sample(eng._h, C.byref(args), args.mem, out.ctypes.data, None) != 0
        assert str(L) in eng.lib.pd_last_error().decode()
        assert eng.lib.pd_sample_begin(eng._h, C.byref(args)) != 0
    with pytest.raises(ValueError, match="must have the shape of ctx_cond"):
        eng.ddim_sample(steps=2, cfg_scale=4.0, **dict(a, ctx_uncond=a["ctx_uncond"][:, :40]))


def test_sessions_of_different_lengths_in_a_row_equal_fresh_engines(net):
    """arena re-sizing (the second session's K / V are larger than the first's) and graph reuse (same shapes and step count,
    another L: a captured loop of the other length must not be replayed)"""
    calls = [(40, 4), (231, 4), (40, 4), (77, 4)]
    fresh = []
    for L, S in calls[:2] + calls[3:]:
        e = E.Engine(W.TINY, precision="f32")
        e.load_state_dict(net[0])
        fresh.append(e.ddim_sample(steps=S, cfg_scale=5.0, **inputs(L, seed=35)))
        e.close()
    want = [fresh[0], fresh[1], fresh[0], fresh[2]]
    for graph in (0, 1):
        e = E.Engine(W.TINY, precision="f32")
        e.load_state_dict(net[0])
        e.set_option("graph", graph)
        try:
            for (L, S), w in zip(calls, want):
                np.testing.assert_array_equal(e.ddim_sample(steps=S, cfg_scale=5.0, **inputs(L, seed=35)), w)
            if graph:
                # every length captures a loop of its own (the second L = 40 call replays, unless the L = 231 session grew the
                # workspace, which drops the captured loops)
                assert e.stat("graph_captures") >= 3 and e.stat("graph_captures") + e.stat("graph_replays") == 4
            # the stepwise session and eps_at honour the length too
            a = inputs(231, seed=35)
            e.sample_begin(steps=4, cfg_scale=5.0, **a)
            for i in range(4):
                e.sample_step(i)
            np.testing.assert_array_equal(e.sample_get(), want[1])
            e.sample_end()
        finally:
            e.close()


@pytest.mark.parametrize("mode", ["guess", "only_mid"])
def test_guess_mode_and_only_mid_control_at_154(eng, net, mode):
    sd, lay = net
    a = inputs(154, B=2, seed=37)
    S, gs = 2, 5.0
    fn = oracle_eps(net, a, gs, guess=mode == "guess", only_mid=mode == "only_mid")
    sched = O.make_schedule(S)
    x, ref = a["x_T"], []
    for i, step in enumerate(np.flip(sched["ddim_timesteps"])):
        index = S - i - 1
        e_t = fn(x, step)
        a_t, a_prev = sched["ddim_alphas"][index], sched["ddim_alphas_prev"][index]
        pred = (x - sched["ddim_sqrt_one_minus_alphas"][index] * e_t) / np.sqrt(a_t)
        x = (np.sqrt(a_prev) * pred + np.sqrt(np.float32(1.0) - a_prev) * e_t).astype(np.float32)
        ref.append(x)
    got, inter = eng.ddim_sample(steps=S, cfg_scale=gs, guess_mode=mode == "guess", only_mid_control=mode == "only_mid",
                                 return_intermediates=True, **a)
    errs = [relerr(inter[i + 1], ref[i]) for i in range(S)]
    print(f"[L 154] {mode}: per-step relerr {['%.2e' % v for v in errs]}")
    assert max(errs) < TRAJ
    # a context of another length without saying so is refused on the Python side whether or not guidance is on
    with pytest.raises(ValueError, match="must have the shape of ctx_cond"):
        eng.ddim_sample(steps=S, cfg_scale=1.0, use_cfg=False, **dict(a, ctx_uncond=a["ctx_uncond"][:, :77]))


def test_eps_takes_any_length(eng, net):
    sd, lay = net
    a = inputs(231, B=2, seed=39)
    t = np.array([500, 20], np.int64)
    ref = O.apply_model(sd, W.TINY, lay, a["x_T"], t, a["ctx_cond"], a["pair"], a["query"])
    assert relerr(eng.eps(a["x_T"], t, a["ctx_cond"], a["pair"], a["query"]), ref) < 1e-4


# ------------------------------------------------------------------------------------------------ through the fused tail
ONE_LEVEL = dataclasses.replace(W.SD15, channel_mult=(1,), num_res_blocks=1, attention_resolutions=(1,), vae_ch=0, text_layers=0)


def test_fused_tail_in_the_sampling_loop_at_231():
    """one level of 320 channels, latent 16 x 16 (256 tokens), B = 1 with CFG, f16, L = 231: the 320-channel blocks take the fused
    tail with three windows; the shared CFG front hands it `in_rows` = half the rows"""
    cfg, B, h, w, L, S = ONE_LEVEL, 1, 16, 16, 231, 3
    inp = W.synth_inputs(cfg, B, h, w, seed=41)
    r = np.random.default_rng(41)
    a = dict(x_T=inp["x_T"], pair=inp["pair"], query=inp["query"], ctx_cond=r.standard_normal((B, L, 768), dtype=np.float32),
             ctx_uncond=r.standard_normal((B, L, 768), dtype=np.float32))
    e = E.Engine(cfg, precision="f16")
    try:
        e.init_random_weights(778)

        def run():
            e.sample_begin(steps=50, cfg_scale=7.5, **a)
            n1 = e.stat("launches")
            lat = []
            for i in range(S):
                e.sample_step(i)
                lat.append(np.array(e.sample_get()))
            flags = e.stat("cfg_shared")
            e.sample_end()
            return lat, e.stat("launches") - n1, flags
        shared, n_fused, flags = run()
        assert flags == 3                                      # UNet and ControlNet fronts shared
        e.set_option("cfg_share", 0)
        doubled, _, flags = run()
        assert flags == 0
        e.set_option("cfg_share", 1)
        e.set_option("st_fuse", 0)
        plain, n_plain, _ = run()
        assert np.isfinite(shared[-1]).all()
        assert n_fused < n_plain, (n_fused, n_plain)          # the per-layer path launches more kernels per step
        errs = [relerr(s, d) for s, d in zip(shared, doubled)]
        print(f"[one level, L 231] cfg_share on vs off per step {['%.2e' % v for v in errs]}")
        errs_f = [relerr(s, p) for s, p in zip(shared, plain)]
        print(f"[one level, L 231] st_fuse on vs off per step {['%.2e' % v for v in errs_f]}, launches {n_fused} / {n_plain}")
        for s, d in zip(shared, doubled):
            np.testing.assert_array_equal(s, d)
        assert max(errs_f) < 5e-3
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ pipeline
def test_pipeline_long_prompts_on_the_engine_clip():
    cfg = W.TINY
    gold = np.load(os.path.join(GOLD, "long_prompt.npz"))
    tok = StubTokenizer(cfg.text_vocab)
    prompts = [prompt_of(n, 100 + i, cfg.text_vocab) for i, n in enumerate(TOKEN_COUNTS)]
    e = E.Engine(cfg, precision="f32")
    try:
        e.load_state_dict(W.synth_state_dict(cfg))
        e.load_state_dict(W.synth_text_state_dict(cfg))
        pipe = PromptDiffusionPipeline(e, tokenizer=tok)
        pipe.enable_long_prompts()
        pe, ne = pipe.encode_prompt(prompts, 1, True, negative_prompt=None)
        want = e.text_encode(gold["window_ids"].reshape(-1, 77)).reshape(len(prompts), 231, cfg.context_dim)
        assert pe.shape == ne.shape == (len(prompts), 231, cfg.context_dim)
        np.testing.assert_array_equal(pe, want)
        # ... which is what the reference's _hacked_clip_forward computed (fp32, other summation order)
        assert relerr(pe, gold["z"]) < 1e-4
        # every prompt gets three windows, the empty negative prompt included: three times the same [BOS, EOS, pad...] window
        np.testing.assert_array_equal(ne[0, :77], ne[0, 154:])
        # the reference's clip_skip = 3 is the engine's 2
        pipe._clip_skip = 2
        pe3, _ = pipe.encode_prompt(prompts[-1:], 1, False)
        assert relerr(pe3[:, gold["z_rows"]], gold["z_ref_clip_skip3"]) < 1e-4
        pipe._clip_skip = None
        # the (L) facade's cond stage: hack_everything -> the same context, with the reference's own clip_skip count
        from prompt_diffusion_amd.ddim import ControlLDM
        model = ControlLDM(e, tokenizer=tok)
        plain = model.get_learned_conditioning(prompts)                  # unhacked FrozenCLIPEmbedder: truncated to 77
        np.testing.assert_array_equal(plain, e.text_encode(np.asarray(tok(prompts, max_length=77)["input_ids"], np.int32)))
        model.hack_everything()
        np.testing.assert_array_equal(model.get_learned_conditioning(prompts), pe)
        for c in (0, 1):
            model.hack_everything(clip_skip=c)
            np.testing.assert_array_equal(model.get_learned_conditioning(prompts[-1]), pe[-1:])
        model.hack_everything(clip_skip=3)
        assert relerr(model.get_learned_conditioning(prompts[-1:])[:, gold["z_rows"]], gold["z_ref_clip_skip3"]) < 1e-4
        # array-likes that are not arrays are converted as before
        lst = e.eps(inp_x := np.zeros((1, 4, 8, 8), np.float32), np.array([10], np.int64), pe[:1].tolist(),
                    np.zeros((1, 6, 64, 64), np.float32), np.zeros((1, 3, 64, 64), np.float32))
        assert lst.shape == inp_x.shape
        # images: prompts in = these embeddings in
        sel = [4, 6]
        inp = W.synth_inputs(cfg, 2, 8, 8, seed=43, unit_range=True)
        pa, pb = inp["pair"][:, :3], inp["pair"][:, 3:]
        kw = dict(image=inp["query"].transpose(0, 2, 3, 1), image_pair=[pa.transpose(0, 2, 3, 1), pb.transpose(0, 2, 3, 1)],
                  num_inference_steps=3, guidance_scale=5.0, latents=inp["x_T"], output_type="latent")
        from_prompts = np.asarray(pipe(prompt=[prompts[i] for i in sel], **kw).images)
        from_embeds = np.asarray(pipe(prompt_embeds=pe[sel], negative_prompt_embeds=ne[sel], **kw).images)
        np.testing.assert_array_equal(from_prompts, from_embeds)
        pipe.disable_long_prompts()
        short = np.asarray(pipe(prompt=[prompts[i] for i in sel], **kw).images)     # truncated to 77 tokens: another context
        assert relerr(short, from_prompts) > 1e-3
    finally:
        e.close()
