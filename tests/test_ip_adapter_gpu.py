"""IP-Adapter on the GPU (tests/ip_adapter_ref.py holds the references; tests/test_ip_adapter_cpu.py shows that the kernel bound has teeth
and that the seeded TINY adapter moves eps by far more than any tolerance here).

1. ip_attn_add_kernel through pd_op_ip_attention_add against its per-element fp64 bound, four modes.
2. One SD1.5 block at C = 320, N = 1024 through pd_op_spatial_transformer_ip against the restatement; scale 0 is the plain call, bit for bit.
3. The TINY network with the adapter against the restatement: eps and the 5-step trajectory, guidance on and off, every mode.
4. Bit-identities on TINY.   5. The pipelines end to end with the tiny image tower.
Each test prints its figures ("[ip] ..." lines, pytest -s)."""
import dataclasses
import functools

import numpy as np
import pytest

from oracle import pd_oracle as O
from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import ip_adapter as IP
from prompt_diffusion_amd import weights as W
from prompt_diffusion_amd.pipeline import PromptDiffusionPipeline
from prompt_diffusion_amd.schedulers import UniPCMultistepScheduler
from tests import attn_ref as R
from tests import clip_vision_ref as CV
from tests import ip_adapter_ref as IR
from tests.test_ip_adapter_cpu import (KERNEL_FAMILIES, KERNEL_SCALES, KERNEL_SHAPES, MODES, TINY_E, TINY_T, kernel_case, tiny_adapter,
                                       tiny_embeds)
from tests.test_st_tail_gpu import BLK, PRE, TOL as BLOCK_TOL, block_weights, make_engine

pytestmark = pytest.mark.gpu
TINY_IP = dataclasses.replace(W.TINY, ip_adapter=(TINY_T, TINY_E))
B, HW, S, CFG_SCALE, T_EPS = 2, 16, 5, 7.5, 801          # the shape of tiny_b2_16x16_s5
NS = 4                                                   # steps of the bit-identity and pipeline calls (8 x 8 latents)


def relerr(a, b):
    return float(np.abs(np.asarray(a) - b).max() / (np.abs(b).max() + 1e-30))


def tiny_engine(prec, adapter=True):
    e = E.Engine(TINY_IP if adapter else W.TINY, precision=prec)
    e.load_state_dict(W.synth_state_dict(W.TINY))
    if adapter:
        e.load_state_dict(tiny_adapter(), strict=False)
        assert e.ip_adapter_weights_missing() == 0
    return e


@pytest.fixture(scope="module")
def eng():
    e = tiny_engine("f32")
    yield e
    e.close()


def sample_kw(inp, **over):
    kw = dict(x_T=inp["x_T"], ctx_cond=inp["ctx_cond"], ctx_uncond=inp["ctx_uncond"], pair=inp["pair"], query=inp["query"], steps=S,
              cfg_scale=CFG_SCALE)
    kw.update(over)
    return kw


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("mode", MODES)
def test_kernel_within_its_bound(mode):
    e = E.Engine(W.TINY, precision=mode)
    worst, fails = (0.0, None), []
    try:
        for shape in KERNEL_SHAPES:
            heads = shape[3]
            for family in KERNEL_FAMILIES:
                for s in KERNEL_SCALES:
                    q, att, k, v, ref, bound = kernel_case(mode, family, shape, s)
                    got = e.op_ip_attention_add(q, att, k, v, heads=heads, s=s)
                    r, at = R.check(got, ref, bound)
                    if r > worst[0]:
                        worst = (r, (shape, family, s, at))
                    if not r <= 1.0:
                        fails.append((shape, family, s, r, at))
    finally:
        e.close()
    print(f"[ip] kernel {mode}: worst err / bound {worst[0]:.3f} at {worst[1]}")
    assert not fails, f"{mode}: err / bound > 1 in {len(fails)} cases: {fails[:6]}"


# ------------------------------------------------------------------------------------------------ 2. one block
@functools.lru_cache(maxsize=None)
def block_case():
    """weights, inputs and both references of the SD1.5 block input_blocks.1.1 (C = 320) at 32 x 32 tokens, batch 1"""
    sd = block_weights()
    ip_sd = {f"ip_adapter.1.{n}.weight": W.synth_tensor(f"ip_adapter.1.{n}.weight", (320, 768), "w", 99) for n in ("to_k_ip", "to_v_ip")}
    g = np.random.default_rng(41)
    x, ctx = g.standard_normal((1, 320, 32, 32), dtype=np.float32), g.standard_normal((1, 77, 768), dtype=np.float32)
    tok = g.standard_normal((1, 4, 768), dtype=np.float32)
    scales = np.zeros(16, np.float32); scales[0] = 0.75
    with IR.ip_active(ip_sd, {BLK: 0}, tok, scales):
        ref = O.spatial_transformer(O.Net(sd, PRE), BLK, x, ctx, heads=8)
    plain = O.spatial_transformer(O.Net(sd, PRE), BLK, x, ctx, heads=8)
    return sd, ip_sd, x, ctx, tok, ref, plain


@pytest.mark.parametrize("prec", MODES)
def test_block_with_the_term_and_scale_zero(prec):
    sd, ip_sd, x, ctx, tok, ref, plain = block_case()
    assert relerr(ref, plain) > 5 * BLOCK_TOL[prec]                   # the term moves the block by more than 5 x the mode's tolerance
    e = make_engine(prec, sd)
    try:
        e.configure_ip_adapter(4, 1024)
        e.load_state_dict(ip_sd, strict=False)
        e.ip_adapter_set_scale(0.75)
        n0 = e.stat("launches"); i0 = e.stat("ip_launches")
        y = e.op_spatial_transformer_ip(PRE + BLK, x, ctx, tok)
        n_on = e.stat("launches") - n0
        assert e.stat("ip_launches") == i0 + 1
        e.ip_adapter_set_scale(0.0)
        n0 = e.stat("launches")
        y0 = e.op_spatial_transformer_ip(PRE + BLK, x, ctx, tok)
        n_zero = e.stat("launches") - n0
        n0 = e.stat("launches")
        yp = e.op_spatial_transformer(PRE + BLK, x, ctx)
        n_plain = e.stat("launches") - n0
    finally:
        e.close()
    print(f"[ip] block {prec}: with the term {relerr(y, ref):.3e}, plain {relerr(yp, plain):.3e} (bound {BLOCK_TOL[prec]:g}); launches "
          f"{n_on} / scale 0 {n_zero} / plain {n_plain}")
    assert relerr(y, ref) < BLOCK_TOL[prec]
    np.testing.assert_array_equal(y0, yp)
    assert n_zero == n_plain and n_on > n_plain
    if prec in ("f16", "bf16"):
        assert n_plain < n_on - 6                                    # the plain call ran the fused tail, the call with the term could not


# ------------------------------------------------------------------------------------------------ 3. the TINY network
@functools.lru_cache(maxsize=None)
def tiny_refs():
    """the restatement on tiny_b2_16x16's inputs, once: eps without guidance (one embedding per sample), the 5-step trajectory under
    guidance (one embedding for every sample, the caller's own negative one) and without (zeros never enter)"""
    cfg = W.TINY
    sd, lay, ip_sd = W.synth_state_dict(cfg), O.make_layouts(cfg, W), tiny_adapter()
    slots, ones = IR.slots_of(IP.block_prefixes(cfg, prefix="")), np.ones(16, np.float32)
    inp = W.synth_inputs(cfg, B, HW, HW)
    cond2, _ = tiny_embeds(B)
    cond1, neg1 = tiny_embeds(1, seed=78)
    cond = dict(c_crossattn=inp["ctx_cond"], example_pair=inp["pair"], query=inp["query"])
    unc = dict(c_crossattn=inp["ctx_uncond"], example_pair=inp["pair"], query=inp["query"])
    t = np.full((B,), T_EPS, np.int64)
    with IR.ip_active(ip_sd, slots, IR.call_tokens(ip_sd, TINY_T, cond2, None, B, False), ones):
        eps = O.apply_model(sd, cfg, lay, inp["x_T"], t, inp["ctx_cond"], inp["pair"], inp["query"])
    with IR.ip_active(ip_sd, slots, IR.call_tokens(ip_sd, TINY_T, cond1, neg1, B, True), ones):
        _, traj_cfg, _ = O.ddim_sampling(sd, cfg, lay, S, inp["x_T"], cond, unc, CFG_SCALE)
    with IR.ip_active(ip_sd, slots, IR.call_tokens(ip_sd, TINY_T, cond1, None, B, False), ones):
        _, traj_one, _ = O.ddim_sampling(sd, cfg, lay, S, inp["x_T"], cond, None, 1.0)
    eps_off = O.apply_model(sd, cfg, lay, inp["x_T"], t, inp["ctx_cond"], inp["pair"], inp["query"])
    return dict(inp=inp, cond2=cond2, cond1=cond1, neg1=neg1, eps=eps, eps_off=eps_off, traj_cfg=np.stack(traj_cfg), traj_one=np.stack(traj_one))


def _network_errors(e, r):
    inp = r["inp"]
    t = np.full((B,), T_EPS, np.int64)
    e.ip_adapter_set_scale(1.0)
    e.ip_adapter_set_image(r["cond2"])
    eps = e.eps(inp["x_T"], t, inp["ctx_cond"], inp["pair"], inp["query"])
    e.ip_adapter_set_image(r["cond1"], r["neg1"])
    _, cfg_inter = e.ddim_sample(**sample_kw(inp), return_intermediates=True)
    e.ip_adapter_set_image(r["cond1"])
    _, one_inter = e.ddim_sample(**sample_kw(inp, use_cfg=False, cfg_scale=1.0), return_intermediates=True)
    e.ip_adapter_clear_image()
    eps_plain = e.eps(inp["x_T"], t, inp["ctx_cond"], inp["pair"], inp["query"])
    return (relerr(eps, r["eps"]), [relerr(cfg_inter[i], r["traj_cfg"][i]) for i in range(S + 1)],
            [relerr(one_inter[i], r["traj_one"][i]) for i in range(S + 1)], relerr(eps_plain, r["eps_off"]))


def test_tiny_network_f32(eng):
    r = tiny_refs()
    assert relerr(r["eps"], r["eps_off"]) > 10 * 1e-4
    e_eps, e_cfg, e_one, e_off = _network_errors(eng, r)
    print(f"[ip] TINY f32: eps {e_eps:.2e} (adapter off {e_off:.2e}); per step with guidance {['%.1e' % v for v in e_cfg]}, without "
          f"{['%.1e' % v for v in e_one]}")
    assert e_eps < 1e-4 and e_off < 1e-4
    assert max(e_cfg) < 2e-4 and max(e_one) < 2e-4


@pytest.mark.parametrize("prec,tol_eps,tol_step", [("bf16", 3e-2, 5e-2), ("f16", 2.5e-3, 5e-3), ("f16x2", 2e-4, 1e-3)])
def test_tiny_network_reduced_precision(prec, tol_eps, tol_step):
    """the bounds of test_network_gpu.py::test_tiny_reduced_precision, unchanged"""
    r = tiny_refs()
    e = tiny_engine(prec)
    try:
        e_eps, e_cfg, e_one, e_off = _network_errors(e, r)
    finally:
        e.close()
    print(f"[ip] TINY {prec}: eps {e_eps:.2e} (adapter off, same inputs {e_off:.2e}; bound {tol_eps:g}); per step with guidance "
          f"{['%.1e' % v for v in e_cfg]}, without {['%.1e' % v for v in e_one]} (bound {tol_step:g})")
    assert e_eps < tol_eps
    assert max(e_cfg) < tol_step and max(e_one) < tol_step


# ------------------------------------------------------------------------------------------------ 4. bit-identities
def test_scale_zero_is_no_adapter(eng):
    """(a) adapter loaded, image set, scale 0: the latents and the launches of an engine that has no adapter"""
    inp = W.synth_inputs(W.TINY, B, 8, 8, seed=31)
    plain = tiny_engine("f32", adapter=False)
    try:
        n0 = plain.stat("launches")
        want = plain.ddim_sample(**sample_kw(inp, steps=NS))
        n_plain = plain.stat("launches") - n0
    finally:
        plain.close()
    eng.ip_adapter_set_image(tiny_embeds(1)[0])
    try:
        eng.ip_adapter_set_scale(0.0)
        n0, i0 = eng.stat("launches"), eng.stat("ip_launches")
        got = eng.ddim_sample(**sample_kw(inp, steps=NS))
        assert (eng.stat("launches") - n0, eng.stat("ip_launches") - i0) == (n_plain, 0)
        np.testing.assert_array_equal(got, want)
        scales = np.zeros(16, np.float32); scales[3] = 1.0           # one block on: two launches per evaluation under guidance
        eng.ip_adapter_set_scale(scales)
        n0, i0 = eng.stat("launches"), eng.stat("ip_launches")
        one = eng.ddim_sample(**sample_kw(inp, steps=NS))
        assert (eng.stat("launches") - n0, eng.stat("ip_launches") - i0) == (n_plain + 2 * NS, 2 * NS)
        assert not np.array_equal(one, want)
    finally:
        eng.ip_adapter_set_scale(1.0)
        eng.ip_adapter_clear_image()
    np.testing.assert_array_equal(eng.ddim_sample(**sample_kw(inp, steps=NS)), want)      # no image set: no adapter either


def test_cfg_share_broadcast_stepwise_and_batch_rule(eng):
    """(b) cfg_share on / off, (d) one embedding for every sample / the same one repeated, (e) sample_step / the fused loop"""
    inp = W.synth_inputs(W.TINY, B, 8, 8, seed=32)
    cond, neg = tiny_embeds(1, seed=5)
    kw = sample_kw(inp, steps=NS)
    try:
        eng.ip_adapter_set_image(cond, neg)
        base = eng.ddim_sample(**kw)
        eng.set_option("cfg_share", 0)
        doubled = eng.ddim_sample(**kw)
        eng.ip_adapter_clear_image()
        off_doubled = eng.ddim_sample(**kw)
        eng.set_option("cfg_share", 1)
        off_shared = eng.ddim_sample(**kw)
        print(f"[ip] cfg_share on vs off: with the adapter {relerr(base, doubled):.2e}, without {relerr(off_shared, off_doubled):.2e}")
        np.testing.assert_array_equal(base, doubled)
        eng.ip_adapter_set_image(np.repeat(cond, B, 0), np.repeat(neg, B, 0))
        np.testing.assert_array_equal(eng.ddim_sample(**kw), base)
        eng.sample_begin(**kw)
        try:
            for i in range(NS):
                eng.sample_step(i)
            step = eng.sample_get(E.PD_GET_LATENTS)
        finally:
            eng.sample_end()
        np.testing.assert_array_equal(step, base)
        # three embeddings for a batch of two: refused with both numbers
        eng.ip_adapter_set_image(np.repeat(cond, 3, 0))
        with pytest.raises(E.PdError, match=r"3 image embeddings .* batch is 2"):
            eng.ddim_sample(**kw)
    finally:
        eng.set_option("cfg_share", 1)
        eng.ip_adapter_clear_image()


def test_captured_loops_follow_scale_and_image(eng):
    """(c) graph = 1 against graph = 0, with a scale change and an image change between captured calls"""
    inp = W.synth_inputs(W.TINY, B, 8, 8, seed=33)
    kw = sample_kw(inp, steps=NS)
    img_a, img_b = tiny_embeds(1, seed=6)[0], tiny_embeds(1, seed=7)[0]
    states = [(img_a, 1.0), (img_a, 0.5), (img_b, 0.5), (img_a, 1.0)]
    try:
        want = []
        for img, s in states:
            eng.ip_adapter_set_scale(s)
            eng.ip_adapter_set_image(img)
            want.append(eng.ddim_sample(**kw))
        assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[2])
        np.testing.assert_array_equal(want[0], want[3])
        eng.set_option("graph", 1)
        c0 = eng.stat("graph_captures")
        for (img, s), w in zip(states, want):
            eng.ip_adapter_set_scale(s)
            eng.ip_adapter_set_image(img)
            np.testing.assert_array_equal(eng.ddim_sample(**kw), w)
            np.testing.assert_array_equal(eng.ddim_sample(**kw), w)              # replayed
        assert eng.stat("graph_captures") == c0 + len(states) and eng.stat("graph_replays") >= len(states)
    finally:
        eng.set_option("graph", 0)
        eng.ip_adapter_set_scale(1.0)
        eng.ip_adapter_clear_image()


# ------------------------------------------------------------------------------------------------ 5. the pipelines
TOWER = dataclasses.replace(CV.CONFIGS["A"][0], prefix=W.IMAGE_ENCODER_PREFIX, stream_f32=True)      # two blocks, proj_dim 64 = TINY_E


@pytest.fixture(scope="module")
def pipe_eng():
    e = E.Engine(dataclasses.replace(W.TINY, clip_vision=(TOWER,)), precision="f32")
    e.load_state_dict(W.synth_state_dict(W.TINY))
    e.load_clip_vision_state_dict(CV.synth_state_dict(TOWER), TOWER.prefix)
    assert e.clip_vision_weights_missing(TOWER.prefix) == 0
    yield e
    e.close()


def call_kw(**over):
    inp = W.synth_inputs(W.TINY, B, 8, 8, seed=21, unit_range=True)
    a, b = inp["pair"][:, :3], inp["pair"][:, 3:]
    kw = dict(prompt_embeds=inp["ctx_cond"], negative_prompt_embeds=inp["ctx_uncond"], image=inp["query"].transpose(0, 2, 3, 1),
              image_pair=[a.transpose(0, 2, 3, 1), b.transpose(0, 2, 3, 1)], guidance_scale=4.0, latents=inp["x_T"], num_inference_steps=NS,
              output_type="latent")
    kw.update(over)
    return kw


@pytest.mark.parametrize("device_images", [False, True])
def test_pipeline_image_equals_its_embeds(pipe_eng, device_images):
    from PIL import Image
    pic = Image.fromarray(CV.synth_pictures((70, 90), seed=CV.SEED + 9)[0])
    pipe = PromptDiffusionPipeline(pipe_eng, image_encoder=True, device_images=device_images)
    with pytest.raises(NotImplementedError, match="ip_adapter_image"):
        pipe(ip_adapter_image=pic, **call_kw())
    pipe.load_ip_adapter(IP.nested(tiny_adapter()))
    try:
        plain = np.asarray(pipe(**call_kw()).images)
        from_image = np.asarray(pipe(ip_adapter_image=pic, **call_kw()).images)
        emb = pipe.encode_image(pic)[0]
        assert emb.shape == (1, TINY_E)
        from_embeds = np.asarray(pipe(ip_adapter_image_embeds=emb, **call_kw()).images)
        np.testing.assert_array_equal(from_image, from_embeds)
        assert relerr(from_image, plain) > 1e-2
        np.testing.assert_array_equal(np.asarray(pipe(**call_kw()).images), plain)           # the call cleared its image
        pipe.set_ip_adapter_scale(0.0)
        np.testing.assert_array_equal(np.asarray(pipe(ip_adapter_image=pic, **call_kw()).images), plain)
    finally:
        pipe.unload_ip_adapter()
    with pytest.raises(NotImplementedError, match="ip_adapter_image"):
        pipe(ip_adapter_image_embeds=emb, **call_kw())


def test_pipeline_paths_agree(pipe_eng):
    """(f) fuse_scheduler=True UniPC against its host plug-in to the tolerance of tests/test_unipc_fused_gpu.py (1e-5 on the f32 engine);
    a callback on the default loop against the fused DDIM loop, bit for bit; [negative ; positive] rows and num_images_per_prompt"""
    emb, neg = tiny_embeds(1, seed=8)
    both = np.concatenate([neg, emb])                    # one image: [negative ; positive]
    both4 = np.concatenate([neg, neg, emb, emb])         # one per sample of the batch of two
    outs = {}
    for name, kw in (("fused", dict(scheduler=UniPCMultistepScheduler(), fuse_scheduler=True)), ("host", dict(scheduler=UniPCMultistepScheduler())),
                     ("ddim", {})):
        pipe = PromptDiffusionPipeline(pipe_eng, **kw)
        pipe.load_ip_adapter(tiny_adapter())
        outs[name] = np.asarray(pipe(ip_adapter_image_embeds=both4, **call_kw()).images)
        outs[name + "_plain"] = np.asarray(pipe(**call_kw()).images)
        if name == "ddim":
            outs["cb"] = np.asarray(pipe(ip_adapter_image_embeds=[both4[:, None]], callback_on_step_end=lambda p, i, t, k: {}, **call_kw()).images)
            one = call_kw()
            one = dict(one, prompt_embeds=one["prompt_embeds"][:1], negative_prompt_embeds=one["negative_prompt_embeds"][:1], image=one["image"][:1],
                       image_pair=[p[:1] for p in one["image_pair"]], num_images_per_prompt=2)
            outs["nipp"] = np.asarray(pipe(ip_adapter_image_embeds=both, **one).images)
            assert outs["nipp"].shape == outs["ddim"].shape
        pipe.unload_ip_adapter()
    err = relerr(outs["fused"], outs["host"])
    print(f"[ip] UniPC fused vs host plug-in with the adapter: {err:.2e}; effect {relerr(outs['fused'], outs['fused_plain']):.2e}")
    assert err <= 1e-5
    for name in ("fused", "host", "ddim"):
        assert relerr(outs[name], outs[name + "_plain"]) > 1e-2, name
    np.testing.assert_array_equal(outs["cb"], outs["ddim"])
