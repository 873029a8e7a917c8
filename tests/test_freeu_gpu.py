"""FreeU (pd_set_freeu, freeu_concat_kernel) on the GPU: the kernel against the NumPy restatement, the UNet and the DDIM loop
against the FreeU oracle, graph capture / state changes / off path, the pipeline's scheduler paths, and per-engine state."""
import numpy as np
import pytest

from oracle import pd_oracle as O
from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import weights as W
from prompt_diffusion_amd.ddim import ControlLDM, DDIMSampler
from prompt_diffusion_amd.pipeline import PromptDiffusionPipeline
from prompt_diffusion_amd.schedulers import UniPCMultistepScheduler
from tests import freeu_ref as FR

pytestmark = pytest.mark.gpu

SD15_FREEU = (0.9, 0.2, 1.5, 1.6)   # the published SD1.5 values


def relerr(a, b):
    return float(np.abs(np.asarray(a) - b).max() / (np.abs(b).max() + 1e-30))


def _engine(prec, cfg=W.TINY):
    e = E.Engine(cfg, precision=prec)
    e.load_state_dict(W.synth_state_dict(cfg))
    return e


def _round_storage(x, prec):
    """the values the engine stores for x in its residual-stream type"""
    x = np.asarray(x, np.float32)
    if prec == "f16":
        return x.astype(np.float16).astype(np.float32)
    if prec == "bf16":
        u = x.view(np.uint32).astype(np.uint64)
        u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16).astype(np.uint32)
        return u.view(np.float32)
    return x


# ----------------------------------------------------------------------------------------------------------------- kernel
@pytest.fixture(scope="module", params=["f32", "f16x2", "f16", "bf16"])
def op_engine(request):
    e = E.Engine(W.TINY, precision=request.param)
    yield request.param, e
    e.close()


def _kernel_case(e, prec, B, Ch, Cs, H, W_, s, b, with_h_add, with_skip_add, skip_half=False, add_half=False, seed=0):
    rng = np.random.default_rng(seed)
    f = lambda *sh: _round_storage(rng.standard_normal(sh).astype(np.float32), prec)
    h = f(B, Ch, H, W_)
    ha = f(B, Ch, H, W_) if with_h_add else None
    sB = B // 2 if skip_half else B
    aB = B // 2 if add_half else B
    sk = f(sB, Cs, H, W_)
    sa = f(aB, Cs, H, W_) if with_skip_add else None
    got = e.op_freeu_concat(h, sk, s, b, h_add=ha, skip_add=sa)
    # reference: the kernel adds the residuals in fp32 and rounds once, at the store; FreeU in float64
    hh = h if ha is None else h + ha
    ss = np.concatenate([sk] * (B // sB))
    if sa is not None:
        ss = ss + np.concatenate([sa] * (B // aB))
    hr, sr = FR.apply_freeu(0, hh, ss, s, 1.0, b, 1.0)
    ref = np.concatenate([hr, sr], axis=1)
    return got, ref


def _check(got, ref, prec):
    assert np.isfinite(got).all()
    if prec in ("f32", "f16x2"):
        assert relerr(got, ref) <= 1e-6, relerr(got, ref)
    else:
        # one rounding to the storage type (half an ulp: 2^-11 f16, 2^-8 bf16) on top of fp32 arithmetic
        half_ulp = 2.0 ** -11 if prec == "f16" else 2.0 ** -8
        bound = half_ulp * np.abs(ref) * 1.0001 + 1e-6 * np.abs(ref).max()
        bad = np.abs(got - ref) > bound
        assert not bad.any(), (prec, float(np.abs(got - ref).max()), int(bad.sum()))


@pytest.mark.parametrize("hw", [(1, 1), (2, 2), (3, 2), (8, 8), (9, 7), (12, 12), (16, 16), (24, 24)])
def test_kernel_matches_numpy(op_engine, hw):
    prec, e = op_engine
    H, W_ = hw
    for i, (Ch, Cs, ha, sa, sh, ah) in enumerate([(64, 32, True, True, False, False), (32, 96, False, False, False, False),
                                                  (128, 64, True, False, True, False), (96, 72, True, True, True, True),
                                                  (64, 64, False, True, False, True)]):
        got, ref = _kernel_case(e, prec, 4, Ch, Cs, H, W_, 0.9, 1.5, ha, sa, sh, ah, seed=i)
        _check(got, ref, prec)


@pytest.mark.parametrize("hw,Cs", [((8, 8), 1280), ((16, 16), 1280), ((16, 16), 640)])
def test_kernel_sd15_shapes(op_engine, hw, Cs):
    """The headline's FreeU concats: Bf 16, C_h 1280, the 8x8 and 16x16 planes, stage 1 / stage 2 values."""
    prec, e = op_engine
    for s, b, half in ((0.9, 1.5, False), (0.2, 1.6, True)):
        got, ref = _kernel_case(e, prec, 16, 1280, Cs, hw[0], hw[1], s, b, True, True, skip_half=half)
        _check(got, ref, prec)


def test_kernel_identity_values_equal_concat(op_engine):
    """s = b = 1 is a plain concat up to fp32 rounding of the (zero) correction."""
    prec, e = op_engine
    got, ref = _kernel_case(e, prec, 2, 32, 32, 5, 3, 1.0, 1.0, True, True)
    _check(got, ref, prec)


# ----------------------------------------------------------------------------------------------------------------- network
_ORACLE = {}


def _net_inputs(h, w):
    inp = W.synth_inputs(W.TINY, 2, h, w, seed=17)
    x_in = np.concatenate([inp["x_T"]] * 2)
    t_in = np.full((4,), 761, np.int64)
    ctx = np.concatenate([inp["ctx_uncond"], inp["ctx_cond"]])
    return x_in, t_in, ctx, np.concatenate([inp["pair"]] * 2), np.concatenate([inp["query"]] * 2)


def _oracle_eps(h, w):
    if (h, w) not in _ORACLE:
        sd = W.synth_state_dict(W.TINY)
        lay = O.make_layouts(W.TINY, W)
        with FR.enabled(*SD15_FREEU):
            _ORACLE[(h, w)] = O.apply_model(sd, W.TINY, lay, *_net_inputs(h, w))
    return _ORACLE[(h, w)]


@pytest.mark.parametrize("prec,tol", [("f32", 1e-4), ("bf16", 3e-2), ("f16", 2.5e-3), ("f16x2", 2e-4)])
@pytest.mark.parametrize("hw", [(16, 16), (32, 24)])
def test_eps_matches_freeu_oracle(prec, tol, hw):
    e = _engine(prec)
    try:
        args = _net_inputs(*hw)
        off = e.eps(*args)
        assert e.freeu is None
        e.set_freeu(*SD15_FREEU)
        assert e.freeu == tuple(float(np.float32(v)) for v in SD15_FREEU)
        on = e.eps(*args)
        ref = _oracle_eps(*hw)
        err = relerr(on, ref)
        print(f"[freeu eps] {prec} {hw}: relerr vs oracle {err:.3e}, on vs off {relerr(on, off):.3e}")
        assert err < tol
        assert relerr(on, off) > 1e-2
        e.disable_freeu()
        assert e.freeu is None
        np.testing.assert_array_equal(e.eps(*args), off)
    finally:
        e.close()


# ----------------------------------------------------------------------------------------------------------------- loop
def test_ddim_loop_graph_state_and_off_path():
    cfg = W.TINY
    inp = W.synth_inputs(cfg, 2, 16, 16, seed=3)
    S, gs = 5, 5.0
    kw = dict(x_T=inp["x_T"], ctx_cond=inp["ctx_cond"], ctx_uncond=inp["ctx_uncond"], pair=inp["pair"], query=inp["query"],
              steps=S, cfg_scale=gs)
    plain = _engine("f32")     # never enables FreeU
    e = _engine("f32")
    try:
        never, never_inter = plain.ddim_sample(return_intermediates=True, **kw)
        n0 = plain.stat("launches")
        plain.ddim_sample(**kw)
        launches_off = plain.stat("launches") - n0

        e.set_freeu(*SD15_FREEU)
        out = e.ddim_sample(**kw)
        n0 = e.stat("launches")
        np.testing.assert_array_equal(e.ddim_sample(**kw), out)
        assert e.stat("launches") - n0 == launches_off
        sd = W.synth_state_dict(cfg)
        lay = O.make_layouts(cfg, W)
        cond = dict(c_crossattn=inp["ctx_cond"], example_pair=inp["pair"], query=inp["query"])
        unc = dict(c_crossattn=inp["ctx_uncond"], example_pair=inp["pair"], query=inp["query"])
        with FR.enabled(*SD15_FREEU):
            _, ref, _ = O.ddim_sampling(sd, cfg, lay, S, inp["x_T"], cond, unc, gs)
        errs = []
        for i in range(S):   # per step: the engine from the oracle's x_i must land on the oracle's x_{i+1}
            e.sample_begin(**kw)
            e.sample_set_latents(ref[i])
            e.sample_step(i)
            errs.append(relerr(e.sample_get(), ref[i + 1]))
            e.sample_end()
        print("[freeu ddim] per-step relerr", ["%.2e" % v for v in errs], "trajectory", "%.2e" % relerr(out, ref[-1]))
        assert max(errs) <= 2e-4
        assert relerr(out, ref[-1]) <= 2e-4
        assert relerr(out, never) > 1e-3

        new = (0.8, 0.3, 1.3, 1.4)
        try:
            e.set_option("graph", 1)
            np.testing.assert_array_equal(e.ddim_sample(**kw), out)     # capture
            np.testing.assert_array_equal(e.ddim_sample(**kw), out)     # replay
            e.set_freeu(*new)
            g_new = e.ddim_sample(**kw)                                  # must not replay the old values
            e.set_option("graph", 0)
            np.testing.assert_array_equal(e.ddim_sample(**kw), g_new)
            assert relerr(g_new, out) > 1e-4
            e.set_option("graph", 1)
            e.disable_freeu()
            np.testing.assert_array_equal(e.ddim_sample(**kw), never)
            for i in range(4):
                v = list(SD15_FREEU)
                v[i] = 0.0
                e.set_freeu(*v)
                np.testing.assert_array_equal(e.ddim_sample(**kw), never)
        finally:
            e.set_option("graph", 0)
        e.set_freeu(*v)
        got, got_inter = e.ddim_sample(return_intermediates=True, **kw)
        np.testing.assert_array_equal(got_inter, never_inter)
        with pytest.raises(E.PdError, match="finite"):
            e.set_freeu(float("nan"), 0.2, 1.5, 1.6)
        with pytest.raises(E.PdError, match="finite"):
            e.set_freeu(0.9, 0.2, float("inf"), 1.6)
        assert e.freeu == tuple(float(np.float32(x)) for x in v)   # a rejected call leaves the state as it was
    finally:
        e.close()
        plain.close()


def test_two_engines_are_isolated():
    inp = W.synth_inputs(W.TINY, 1, 16, 16, seed=9)
    kw = dict(x_T=inp["x_T"], ctx_cond=inp["ctx_cond"], ctx_uncond=inp["ctx_uncond"], pair=inp["pair"], query=inp["query"],
              steps=4, cfg_scale=5.0)
    a, b = _engine("f16"), _engine("f16")
    try:
        before = b.ddim_sample(**kw)
        a_off = a.ddim_sample(**kw)
        a.set_freeu(*SD15_FREEU)
        a_on = a.ddim_sample(**kw)
        assert b.freeu is None
        np.testing.assert_array_equal(b.ddim_sample(**kw), before)
        assert relerr(a_on, a_off) > 1e-3
        b.set_freeu(*SD15_FREEU)
        assert relerr(b.ddim_sample(**kw), a_on) < 1e-6
    finally:
        a.close()
        b.close()


# ----------------------------------------------------------------------------------------------------------------- pipeline
@pytest.fixture(scope="module")
def eng():
    e = _engine("f32")
    yield e
    e.close()


def _pipe_kw(B=2, hw=64, seed=11, **over):
    inp = W.synth_inputs(W.TINY, B, hw // 8, hw // 8, seed=seed, unit_range=True)
    a, b = inp["pair"][:, :3], inp["pair"][:, 3:]
    kw = dict(prompt_embeds=inp["ctx_cond"], negative_prompt_embeds=inp["ctx_uncond"], image=inp["query"].transpose(0, 2, 3, 1),
              image_pair=[a.transpose(0, 2, 3, 1), b.transpose(0, 2, 3, 1)], guidance_scale=5.0, latents=inp["x_T"],
              output_type="latent")
    kw.update(over)
    return kw, inp


def test_pipeline_enable_freeu_default_ddim_and_callback_path(eng):
    from tests.test_pipeline_gpu import _oracle_pipeline
    cfg, S = W.TINY, 4
    kw, inp = _pipe_kw(num_inference_steps=S, controlnet_conditioning_scale=0.8)
    pipe = PromptDiffusionPipeline(eng)
    off = np.asarray(pipe(**kw).images)
    pipe.enable_freeu(*SD15_FREEU)
    try:
        assert eng.freeu is not None
        on = np.asarray(pipe(**kw).images)
        seen = []
        stepwise = np.asarray(pipe(callback_on_step_end=lambda p, i, t, k: seen.append(i) or {}, **kw).images)
        assert seen == list(range(S))
        np.testing.assert_array_equal(stepwise, on)
        sd = W.synth_state_dict(cfg)
        lay = O.make_layouts(cfg, W)
        with FR.enabled(*SD15_FREEU):
            ref = _oracle_pipeline(cfg, sd, lay, inp["x_T"], inp["ctx_cond"], inp["ctx_uncond"], inp["pair"], inp["query"], S, 5.0,
                                   0.8, False, 0.0, 1.0)
        print(f"[freeu pipeline] relerr vs oracle {relerr(on, ref):.3e}, on vs off {relerr(on, off):.3e}")
        assert relerr(on, ref) < 3e-4
        assert relerr(on, off) > 1e-3
    finally:
        pipe.disable_freeu()
    assert eng.freeu is None
    np.testing.assert_array_equal(np.asarray(pipe(**kw).images), off)


def test_pipeline_unipc_fused_matches_host_with_freeu(eng):
    kw, _ = _pipe_kw(num_inference_steps=5, controlnet_conditioning_scale=0.9, guidance_scale=4.0, seed=21)
    sk = dict(solver_order=2, solver_type="bh2", disable_corrector=[1])

    def run(fused):
        pipe = PromptDiffusionPipeline(eng, scheduler=UniPCMultistepScheduler(**sk), fuse_scheduler=fused)
        seen = []
        out = np.asarray(pipe(callback_on_step_end=lambda p, i, t, k: seen.append(np.array(k["latents"])) or {}, **kw).images)
        return out, seen, pipe

    off, _, _ = run(True)
    eng.set_freeu(*SD15_FREEU)
    try:
        host, hs, _ = run(False)
        fused, fs, pipe = run(True)
        assert len(hs) == len(fs) == 5
        for i, (f, h) in enumerate(zip(fs, hs)):
            assert relerr(f, h) <= 1e-5, (i, relerr(f, h))
        np.testing.assert_array_equal(np.asarray(pipe(**kw).images), fused)   # pd_unipc_sample without callbacks
        assert relerr(fused, off) > 1e-3
    finally:
        eng.disable_freeu()


def test_ddim_sampler_facade_applies_engine_freeu(eng):
    """The (L) DDIMSampler facade evaluates the UNet on the same engine, so FreeU applies there too."""
    inp = W.synth_inputs(W.TINY, 2, 16, 16, seed=13)
    S = 4
    cond = {"c_crossattn": [inp["ctx_cond"]], "example_pair": [inp["pair"]], "query": [inp["query"]]}
    uc = {"c_crossattn": [inp["ctx_uncond"]], "example_pair": [inp["pair"]], "query": [inp["query"]]}
    sampler = DDIMSampler(ControlLDM(eng))
    kw = dict(x_T=inp["x_T"], ctx_cond=inp["ctx_cond"], ctx_uncond=inp["ctx_uncond"], pair=inp["pair"], query=inp["query"],
              steps=S, cfg_scale=6.0)
    eng.set_freeu(*SD15_FREEU)
    try:
        samples, _ = sampler.sample(S, 2, (4, 16, 16), cond, eta=0.0, x_T=inp["x_T"], unconditional_guidance_scale=6.0,
                                    unconditional_conditioning=uc, verbose=False)
        assert relerr(samples, eng.ddim_sample(**kw)) < 1e-6
    finally:
        eng.disable_freeu()
    assert relerr(samples, eng.ddim_sample(**kw)) > 1e-3
