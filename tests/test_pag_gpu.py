"""Perturbed-attention guidance (pd_set_pag) on the GPU, against the NumPy restatement of tests/pag_ref.py.
1. pag_identity_kernel (csrc/pag.hip) is the NumPy transposition, bit for bit, in every storage type.
2. pd_op_cfg_combine (the guidance of cfg_update_kernel) against the fp32 NumPy restatement, bit for bit.
3. One SD1.5 block (C = 320, 32 x 32 tokens) with its last sample perturbed, within TOL of tests/test_st_tail_gpu.py.
4. The TINY network at B = 2, 16 x 16: eps at t = 801 and the 5-step DDIM trajectory, with and without CFG, within the bounds of
   tests/test_cfg_share_gpu.py (the layer sets and that they have teeth: tests/test_pag_cpu.py).
5. Identities: off is off, fork against the plain evaluation, graphs, the stepwise session, fused UniPC, guess mode, IP-Adapter, the
   adaptive scale.
6. The pipelines.

Test 2 and the arithmetic of an engine without PAG.  pd_op_cfg_combine launches the update kernel as an evaluation with the PAG state on
launches it: the guidance block is compiled with FMA contraction off and every operation is rounded on its own, at every pag_scale -- 0
included, which in the engine is a step at the clamp of the adaptive scale.  An evaluation with the state OFF does not take that block:
it runs the CFG line of every earlier build, whose multiply-add hipcc contracts into one FMA, and that line differs from the separately
rounded NumPy formula in the last bits (87 of 296 fp32 elements of this test's inputs, at most 1.9e-6, measured when the op ran it).  The
issue asks both for that path to stay exactly as it is and for bit-equality with NumPy at pag_scale 0; the first is kept for the engine
(test_off_is_off, and the parent comparison of profiles/pag_dispatch_equal.txt), the second holds for the guidance of PAG evaluations."""
import dataclasses
import functools

import numpy as np
import pytest

from oracle import pd_oracle as O
from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import ip_adapter as IP
from prompt_diffusion_amd import weights as W
from prompt_diffusion_amd.pag import parse_pag_layers
from prompt_diffusion_amd.pipeline import PromptDiffusionImg2ImgPipeline, PromptDiffusionInpaintPipeline, PromptDiffusionPipeline
from prompt_diffusion_amd.schedulers import UniPCMultistepScheduler
from tests import ip_adapter_ref as IR
from tests import pag_ref as PR
from tests.test_ip_adapter_cpu import TINY_E, TINY_T, tiny_adapter, tiny_embeds
from tests.test_pag_cpu import ALL, B, CFG_SCALE, HW, MID, PAG_SCALE, S, T_EPS, TOL_ORACLE, TOL_PATH, WIDE, conds, tiny
from tests.test_st_tail_gpu import BLK, PRE, TOL as BLOCK_TOL, block_weights, make_engine

pytestmark = pytest.mark.gpu
MODES = ["f32", "f16x2", "f16", "bf16"]
NS = 4      # steps of the identity calls


def relerr(a, b):
    return float(np.abs(np.asarray(a) - b).max() / (np.abs(b).max() + 1e-30))


def mask_of(blocks):
    return sum(1 << j for j in blocks)


def tiny_engine(prec, cfg=W.TINY):
    e = E.Engine(cfg, precision=prec)
    e.load_state_dict(W.synth_state_dict(W.TINY))
    return e


@pytest.fixture(scope="module")
def eng():
    e = tiny_engine("f32")
    yield e
    e.close()


def sample_kw(inp, steps=S, **over):
    kw = dict(x_T=inp["x_T"], ctx_cond=inp["ctx_cond"], ctx_uncond=inp["ctx_uncond"], pair=inp["pair"], query=inp["query"], steps=steps,
              cfg_scale=CFG_SCALE)
    kw.update(over)
    return kw


# ------------------------------------------------------------------------------------------------ 1. the identity kernel
@pytest.mark.parametrize("prec", MODES)
def test_identity_kernel_is_the_transposition(prec):
    e = E.Engine(W.TINY, precision=prec)
    r = np.random.default_rng(11)
    try:
        p0 = e.stat("pag_launches")
        for N in (3, 4, 64, 200, 1024):
            for C in (64, 320, 1280):
                vt = (r.integers(-255, 256, (3, C, N)) / 256.0).astype(np.float32)      # 8 significant bits: exact in f32, f16 and bf16
                got = e.op_pag_identity(vt, 1, 2)
                assert np.array_equal(got, vt[1:3].transpose(0, 2, 1)), (prec, N, C)
        assert e.stat("pag_launches") == p0 + 15
        assert np.array_equal(e.op_pag_identity(vt, 0, 3), vt.transpose(0, 2, 1))
        with pytest.raises(E.PdError):
            e.op_pag_identity(vt, 2, 2)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 2. the guidance
def _round_to(a, dt):
    if dt == E.PD_DT_F16:
        return a.astype(np.float16).astype(np.float32)
    if dt == E.PD_DT_BF16:
        u = a.view(np.uint32).astype(np.uint64)
        u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
        return u.astype(np.uint32).view(np.float32)
    return a


@pytest.mark.parametrize("p", [0.0, 3.0, 0.37])
@pytest.mark.parametrize("dt", [E.PD_DT_F32, E.PD_DT_F16, E.PD_DT_BF16])
@pytest.mark.parametrize("use_cfg", [True, False])
def test_cfg_combine_is_the_numpy_restatement(eng, use_cfg, dt, p):
    b, hw, c = 2, 37, 4
    nb = 2 if use_cfg else 1
    eps = _round_to(np.random.default_rng(5).standard_normal(((nb + 1) * b, hw, c)).astype(np.float32), dt)
    e_u = eps[:b] if use_cfg else None
    e_c, e_p = eps[(nb - 1) * b:nb * b], eps[nb * b:]
    ref = PR.guide(e_u, e_c, e_p, CFG_SCALE, p)
    got = eng.op_cfg_combine(eps if p else eps[:nb * b], b, use_cfg, CFG_SCALE, p, dt)
    print(f"[pag] cfg_combine cfg {use_cfg} dt {dt} p {p}: {int((got != ref).sum())} of {ref.size} elements differ from NumPy, "
          f"max {np.abs(got - ref).max():.2e}")
    assert np.array_equal(got, ref)


# ------------------------------------------------------------------------------------------------ 3. one SD1.5 block
@functools.lru_cache(maxsize=None)
def block_case():
    sd = block_weights()
    r = np.random.default_rng(5)
    x, ctx = r.standard_normal((2, 320, 32, 32), dtype=np.float32), r.standard_normal((2, 77, 768), dtype=np.float32)
    ref = PR.spatial_transformer_pag(sd, PRE + BLK, x, ctx, 8, 1)
    plain = O.spatial_transformer(O.Net(sd, PRE), BLK, x, ctx, heads=8)
    return sd, x, ctx, ref, plain


@pytest.mark.parametrize("prec", MODES)
def test_block_with_a_perturbed_sample(prec):
    sd, x, ctx, ref, plain = block_case()
    assert np.array_equal(ref[0], plain[0])
    assert relerr(ref[1], plain[1]) > 5 * BLOCK_TOL[prec]
    e = make_engine(prec, sd)
    try:
        p0 = e.stat("pag_launches")
        y = e.op_spatial_transformer_pag(PRE + BLK, x, ctx, 1)
        assert e.stat("pag_launches") == p0 + 2          # the identity, and the cross-attention of the perturbed sample
        err, off = relerr(y, ref), relerr(y[1], plain[1])
        print(f"[pag] block {prec}: against the restatement {err:.2e} (bound {BLOCK_TOL[prec]}); perturbed sample against its unperturbed self {off:.2e}")
        assert np.isfinite(y).all() and err < BLOCK_TOL[prec]
        assert off > 5 * BLOCK_TOL[prec]
        with pytest.raises(E.PdError):
            e.op_spatial_transformer_pag(PRE + BLK, x, ctx, 2)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 4. the TINY network
@functools.lru_cache(maxsize=None)
def net_ref(blocks, b, h, w, with_cfg, steps=S, guess=False, adaptive=0.0):
    cfg, sd, lay = tiny()
    inp = W.synth_inputs(cfg, b, h, w)
    cond, unc = conds(inp)
    unc = unc if with_cfg else None
    e_u, e_c, e_p = PR.eps_branches(sd, cfg, lay, W, inp["x_T"], T_EPS, cond, unc, list(blocks), guess)
    eps = PR.guide(e_u, e_c, e_p, CFG_SCALE, PR.pag_scale_at(PAG_SCALE, adaptive, T_EPS))
    traj = PR.ddim_pag(sd, cfg, lay, W, steps, inp["x_T"], cond, unc, CFG_SCALE, PAG_SCALE, list(blocks), adaptive, guess_mode=guess)
    return inp, eps, traj


def _net_errors(e, blocks, b, h, w, with_cfg, steps=S, adaptive=0.0, **over):
    inp, eps_ref, traj = net_ref(blocks, b, h, w, with_cfg, steps, bool(over.get("guess_mode")), adaptive)
    kw = sample_kw(inp, steps, use_cfg=with_cfg, **over)
    e.set_pag(PAG_SCALE, blocks, adaptive)
    try:
        e.sample_begin(**kw)
        eps = e.sample_eps_at(T_EPS)
        e.sample_end()
        _, inter = e.ddim_sample(return_intermediates=True, **kw)
    finally:
        e.disable_pag()
    return relerr(eps, eps_ref), [relerr(inter[i + 1], traj[i]) for i in range(steps)]


@pytest.mark.parametrize("with_cfg", [True, False])
@pytest.mark.parametrize("prec", MODES)
def test_tiny_network(prec, with_cfg):
    e = tiny_engine(prec)
    try:
        for blocks in ([MID, WIDE] if prec in ("f32", "f16x2") else [WIDE]):
            e_eps, e_traj = _net_errors(e, blocks, B, HW, HW, with_cfg)
            print(f"[pag] TINY {prec} cfg {with_cfg} blocks {blocks[:3]}..: eps {e_eps:.2e}, per step {['%.1e' % v for v in e_traj]} (bound {TOL_ORACLE[prec]})")
            assert e_eps < TOL_ORACLE[prec] and max(e_traj) < TOL_ORACLE[prec]
            assert e.stat("pag_fork_block") == (15 if blocks == MID else 0)
    finally:
        e.close()


def test_tiny_network_odd_tokens(eng):
    """B = 1, 8 x 24 latents, every block perturbed: token counts 192, 48, 12 and N = 3 in the middle block"""
    e_eps, e_traj = _net_errors(eng, ALL, 1, 8, 24, True)
    print(f"[pag] TINY f32 1 x 8 x 24, all blocks: eps {e_eps:.2e}, per step {['%.1e' % v for v in e_traj]}")
    assert e_eps < TOL_ORACLE["f32"] and max(e_traj) < TOL_ORACLE["f32"]


# ------------------------------------------------------------------------------------------------ 5. identities
def test_off_is_off(eng):
    inp = W.synth_inputs(W.TINY, B, 8, 8, seed=31)
    kw = sample_kw(inp, NS)
    fresh = tiny_engine("f32")
    try:
        n0 = fresh.stat("launches")
        ref = fresh.ddim_sample(**kw)
        n_plain = fresh.stat("launches") - n0
        assert fresh.pag is None and fresh.stat("pag_launches") == 0
    finally:
        fresh.close()
    eng.set_pag(PAG_SCALE, WIDE)
    assert eng.pag == (PAG_SCALE, 0.0, mask_of(WIDE))
    on = eng.ddim_sample(**kw)
    assert not np.array_equal(on, ref)
    for off in ((0.0, WIDE), (PAG_SCALE, 0)):
        eng.set_pag(PAG_SCALE, WIDE)
        eng.set_pag(*off)
        assert eng.pag is None
        n0, p0 = eng.stat("launches"), eng.stat("pag_launches")
        got = eng.ddim_sample(**kw)
        assert np.array_equal(got, ref)
        assert (eng.stat("launches") - n0, eng.stat("pag_launches") - p0) == (n_plain, 0)
    for bad in ((-1.0, 1, 0.0), (float("nan"), 1, 0.0), (3.0, 1, -1.0), (3.0, 1, float("inf")), (3.0, 1 << 16, 0.0)):
        with pytest.raises(E.PdError, match="pd_set_pag"):
            eng.set_pag(*bad)
    assert eng.pag is None


@pytest.mark.parametrize("prec", MODES)
def test_fork_against_the_plain_evaluation(prec):
    """pag_fork 1 against 0, cfg_share 1 against 0 with block 0 in the set, and "mid" at 8 x 8 (a mathematical no-op) against PAG off"""
    inp = W.synth_inputs(W.TINY, B, HW, HW, seed=32)
    small = W.synth_inputs(W.TINY, B, 8, 8, seed=33)
    e = tiny_engine(prec)
    try:
        out = {}
        for blocks in ((MID, WIDE) if prec in ("f32", "f16x2") else (WIDE,)):      # ("mid" alone has no teeth in the 16-bit modes)
            for fork, share in ((1, 1), (0, 1), (1, 0), (0, 0)):
                e.set_option("pag_fork", fork)
                e.set_option("cfg_share", share)
                e.set_pag(PAG_SCALE, blocks)
                out[blocks, fork, share] = e.ddim_sample(**sample_kw(inp, NS))
                assert e.stat("pag_fork_block") == (-1 if not fork else 15 if blocks == MID else 0)
            for k in ((0, 1), (1, 0), (0, 0)):
                err = relerr(out[(blocks,) + k], out[blocks, 1, 1])
                print(f"[pag] {prec} blocks {blocks[:2]}.. fork/share {k} against 1/1: {err:.2e} (bound {TOL_PATH[prec]})")
                assert err < TOL_PATH[prec]
        e.set_option("pag_fork", 1)
        e.set_option("cfg_share", 1)
        e.set_pag(PAG_SCALE, MID)
        a = e.ddim_sample(**sample_kw(small, NS))
        e.disable_pag()
        b = e.ddim_sample(**sample_kw(small, NS))
        print(f"[pag] {prec} 'mid' at 8 x 8 against off: {relerr(a, b):.2e}")
        assert relerr(a, b) < TOL_PATH[prec]
    finally:
        e.close()


def test_graph_and_stepwise(eng):
    inp = W.synth_inputs(W.TINY, B, 8, 8, seed=34)
    kw = sample_kw(inp, NS)
    states = [(PAG_SCALE, WIDE), (1.5, WIDE), (1.5, MID + (6,)), (0.0, WIDE)]
    ref = []
    for s, blocks in states:
        eng.set_pag(s, blocks)
        ref.append(eng.ddim_sample(**kw))
    assert not np.array_equal(ref[0], ref[1]) and not np.array_equal(ref[1], ref[2]) and not np.array_equal(ref[2], ref[3])
    # the stepwise session is the fused loop
    eng.set_pag(PAG_SCALE, WIDE)
    eng.sample_begin(**kw)
    with pytest.raises(E.PdError, match="session"):
        eng.set_pag(2.0, WIDE)
    with pytest.raises(E.PdError, match="session"):
        eng.set_option("pag_fork", 0)
    for i in range(NS):
        eng.sample_step(i)
    step = eng.sample_get()
    eng.sample_end()
    assert np.array_equal(step, ref[0])
    eng.set_option("graph", 1)
    try:
        c0 = eng.stat("graph_captures")
        for (s, blocks), r in zip(states + states[:1], ref + ref[:1]):
            eng.set_pag(s, blocks)
            assert np.array_equal(eng.ddim_sample(**kw), r)       # captured
            assert np.array_equal(eng.ddim_sample(**kw), r)       # replayed
        assert eng.stat("graph_captures") == c0 + 5               # every change of the state dropped the graphs
    finally:
        eng.set_option("graph", 0)
        eng.disable_pag()


def _pipe_kw(inp, **over):
    a, b = inp["pair"][:, :3], inp["pair"][:, 3:]
    kw = dict(prompt_embeds=inp["ctx_cond"], negative_prompt_embeds=inp["ctx_uncond"], image=inp["query"].transpose(0, 2, 3, 1),
              image_pair=[a.transpose(0, 2, 3, 1), b.transpose(0, 2, 3, 1)], guidance_scale=CFG_SCALE, latents=inp["x_T"], output_type="latent",
              num_inference_steps=NS)
    kw.update(over)
    return kw


def test_fused_unipc_against_its_host_plugin(eng):
    inp = W.synth_inputs(W.TINY, B, 8, 8, seed=35, unit_range=True)
    out = {}
    for fused in (False, True):
        pipe = PromptDiffusionPipeline(eng, scheduler=UniPCMultistepScheduler(solver_order=2), fuse_scheduler=fused, pag_applied_layers=["mid", "up", "down.block_0"])
        out[fused] = np.asarray(pipe(pag_scale=PAG_SCALE, **_pipe_kw(inp, num_inference_steps=5)).images)
        out[fused, "off"] = np.asarray(pipe(**_pipe_kw(inp, num_inference_steps=5)).images)
        assert eng.pag is None
    err = relerr(out[True], out[False])
    print(f"[pag] fused UniPC against the host plug-in: {err:.2e}")
    assert err <= 1e-5                                    # the bound of tests/test_unipc_fused_gpu.py
    assert relerr(out[True], out[True, "off"]) > 1e-2


def test_guess_mode(eng):
    e_eps, e_traj = _net_errors(eng, WIDE, B, HW, HW, True, guess_mode=True)
    print(f"[pag] TINY f32 guess mode: eps {e_eps:.2e}, per step {['%.1e' % v for v in e_traj]}")
    assert e_eps < TOL_ORACLE["f32"] and max(e_traj) < TOL_ORACLE["f32"]


def test_adaptive_scale(eng):
    """scale 3.0, adaptive 0.004 over a 10-step grid: p_i = 3 - 0.004 (1000 - t_i) falls to the clamp from t = 201 on"""
    e_eps, e_traj = _net_errors(eng, WIDE, B, HW, HW, True, steps=10, adaptive=0.004)
    print(f"[pag] TINY f32 adaptive scale: eps {e_eps:.2e}, per step {['%.1e' % v for v in e_traj]}")
    assert e_eps < TOL_ORACLE["f32"] and max(e_traj) < TOL_ORACLE["f32"]
    grid = np.flip(O.make_schedule(10, 0.0)["ddim_timesteps"])
    p = [float(PR.pag_scale_at(PAG_SCALE, 0.004, t)) for t in grid]
    assert p[0] > 2.5 and p[-1] == 0.0 and sorted(p, reverse=True) == p, p      # the grid crosses the clamp


def test_ip_adapter_with_pag():
    cfg = dataclasses.replace(W.TINY, ip_adapter=(TINY_T, TINY_E))
    sd, lay, ip_sd = W.synth_state_dict(W.TINY), O.make_layouts(W.TINY, W), tiny_adapter()
    inp = W.synth_inputs(W.TINY, B, HW, HW)
    cond, unc = conds(inp)
    c1, n1 = tiny_embeds(1, seed=78)
    slots, ones = IR.slots_of(IP.block_prefixes(W.TINY, prefix="")), np.ones(16, np.float32)
    tok = IR.call_tokens(ip_sd, TINY_T, c1, n1, B, True)
    tok3 = np.concatenate([tok, tok[B:]])                   # [u ; c ; p]: the perturbed branch reads the conditional tokens
    with IR.ip_active(ip_sd, slots, tok3, ones):
        ref = PR.ddim_pag(sd, W.TINY, lay, W, S, inp["x_T"], cond, unc, CFG_SCALE, PAG_SCALE, list(WIDE))
    e = tiny_engine("f32", cfg)
    try:
        e.load_state_dict(ip_sd, strict=False)
        e.ip_adapter_set_scale(1.0)
        e.ip_adapter_set_image(c1, n1)
        e.set_pag(PAG_SCALE, WIDE)
        _, inter = e.ddim_sample(return_intermediates=True, **sample_kw(inp))
        errs = [relerr(inter[i + 1], ref[i]) for i in range(S)]
        e.set_pag(PAG_SCALE, MID)                           # an unperturbed block with a term behind the fork
        with IR.ip_active(ip_sd, slots, tok3, ones):
            ref_mid = PR.ddim_pag(sd, W.TINY, lay, W, S, inp["x_T"], cond, unc, CFG_SCALE, PAG_SCALE, list(MID), steps_limit=2)
        _, inter = e.ddim_sample(return_intermediates=True, **sample_kw(inp))
        errs_mid = [relerr(inter[i + 1], ref_mid[i]) for i in range(2)]
    finally:
        e.close()
    print(f"[pag] TINY f32 with the IP-Adapter: per step {['%.1e' % v for v in errs]}; 'mid': {['%.1e' % v for v in errs_mid]}")
    assert max(errs) < TOL_ORACLE["f32"] and max(errs_mid) < TOL_ORACLE["f32"]


# ------------------------------------------------------------------------------------------------ 6. the pipelines
def test_pipelines(eng):
    inp = W.synth_inputs(W.TINY, B, 8, 8, seed=36, unit_range=True)
    layers = ["down.block_2", "mid", "up.block_1"]
    pipe = PromptDiffusionPipeline(eng, pag_applied_layers=layers)
    # the default is off: the output and the launches of the call on an engine that never heard of PAG
    fresh = tiny_engine("f32")
    try:
        n0 = fresh.stat("launches")
        plain = np.asarray(PromptDiffusionPipeline(fresh)(**_pipe_kw(inp)).images)
        n_plain = fresh.stat("launches") - n0
    finally:
        fresh.close()
    n0, p0 = eng.stat("launches"), eng.stat("pag_launches")
    off = np.asarray(pipe(**_pipe_kw(inp)).images)
    assert np.array_equal(off, plain) and (eng.stat("launches") - n0, eng.stat("pag_launches") - p0) == (n_plain, 0)
    # pag_scale = 3: the engine-level call with the parsed mask; the engine's own state comes back afterwards
    eng.set_pag(1.25, [3], 0.5)
    got = np.asarray(pipe(pag_scale=PAG_SCALE, **_pipe_kw(inp)).images)
    assert eng.pag == (1.25, 0.5, 1 << 3)
    assert pipe.do_perturbed_attention_guidance and pipe.pag_scale == PAG_SCALE
    eng.set_pag(PAG_SCALE, parse_pag_layers(layers, W.TINY))      # the engine-level state under a call that passes no pag_scale
    want = np.asarray(pipe(**_pipe_kw(inp)).images)
    assert eng.pag == (PAG_SCALE, 0.0, parse_pag_layers(layers, W.TINY))
    assert np.array_equal(got, want) and not np.array_equal(got, plain)
    # ... also after a call that raised inside the engine
    eng.set_pag(1.25, [3], 0.5)
    with pytest.raises(Exception):
        pipe(pag_scale=PAG_SCALE, **_pipe_kw(inp, latents=inp["x_T"][:, :, :7]))
    assert eng.pag == (1.25, 0.5, 1 << 3)
    eng.disable_pag()
    # img2img and inpainting run it
    z0 = np.random.default_rng(7).standard_normal(inp["x_T"].shape).astype(np.float32)
    mask = np.zeros((B, 64, 64), np.float32)
    mask[:, :32] = 1.0
    for cls, extra in ((PromptDiffusionImg2ImgPipeline, dict(strength=0.75)), (PromptDiffusionInpaintPipeline, dict(mask_image=mask, strength=1.0))):
        p = cls(eng, pag_applied_layers=layers)
        kw = _pipe_kw(inp)
        kw["control_image"] = kw.pop("image")
        a = np.asarray(p(image=z0, pag_scale=PAG_SCALE, **extra, **kw).images)
        b = np.asarray(p(image=z0, **extra, **kw).images)
        assert np.isfinite(a).all() and relerr(a, b) > 1e-3 and eng.pag is None
