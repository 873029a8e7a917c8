"""The call frame of the models that run outside the sampling loop (pd_engine::side_call: VAE, HED, M-LSD, the text and image
encoders, the safety checker) -- what no per-model test holds: the side workspace grows with the call and a smaller call afterwards
computes the same bits in it; captured step loops are dropped when it is reallocated and captured again; a NumPy caller and a CUDA
caller get the same bits; a refused call leaves the engine as it was.

Everything here is an equality, so there are no tolerances.  The networks are the tiny ones of the per-model tests, in f32."""
import dataclasses

import numpy as np
import pytest

from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import sd3
from prompt_diffusion_amd import weights as W
from tests import clip_vision_ref as CR

pytestmark = pytest.mark.gpu

TOWER = CR.CONFIGS["A"][0]          # the safety tower of test_clip_vision_gpu.py
CFG = dataclasses.replace(W.TINY, hed=True, mlsd=True, clip_vision=(TOWER,), safety_checker=True)
TCFG = sd3.SD3_TINY_TEXT
NET3 = sd3.SD3Config(in_channels=4, out_channels=4, heads=2, head_dim=64, layers=2, cn_layers=1, joint_dim=TCFG.joint_dim,
                     pooled_dim=TCFG.pooled_dim, pos_embed_max_size=12, cn_pos_embed_max_size=10)
B, H, Wd, S = 1, 16, 16, 5          # the captured loop: 16x16 latents, 5 steps


def make_engine():
    e = E.Engine(CFG, precision="f32")
    for sd in (W.synth_state_dict(W.TINY), W.synth_vae_state_dict(W.TINY), W.synth_text_state_dict(W.TINY)):
        e.load_state_dict(sd, strict=False)
    e.load_hed_state_dict(W.synth_hed_state_dict())
    e.load_mlsd_state_dict(W.synth_mlsd_state_dict())
    e.load_clip_vision_state_dict({**CR.synth_state_dict(TOWER), **{"safety_checker." + k: v for k, v in CR.synth_safety().items() if k != "embeds"}},
                                  TOWER.prefix)
    assert e.weights_missing() == 0 and e.vae_weights_missing() == 0 and e.text_weights_missing() == 0
    assert e.hed_weights_missing() == 0 and e.mlsd_weights_missing() == 0
    assert e.safety_weights_missing() == 0 and e.clip_vision_weights_missing(TOWER.prefix) == 0
    return e


@pytest.fixture(scope="module")
def eng():
    e = make_engine()
    yield e
    e.close()


def make_engine3():
    e = sd3.SD3Engine(NET3, precision="f32")
    e.configure_text(TCFG)
    e.load_state_dict(sd3.synth_sd3_text_state_dict(TCFG, 1234), strict=False)
    assert e.text_weights_missing() == 0
    return e


@pytest.fixture(scope="module")
def eng3():
    e = make_engine3()
    yield e
    e.close()


def pictures(shape, seed):
    return np.random.default_rng(seed).uniform(0.0, 1.0, shape).astype(np.float32)


def sample_kw():
    i = W.synth_inputs(W.TINY, B, H, Wd)
    return dict(x_T=i["x_T"], ctx_cond=i["ctx_cond"], ctx_uncond=i["ctx_uncond"], pair=i["pair"], query=i["query"], steps=S, cfg_scale=4.0)


# ------------------------------------------------------------------------------------------------ grow and return
def grow_and_return(call, stat):
    """call(small), call(large), call(small): the third result is the first bit for bit; the workspace grows at the second call (its
    capacity is always the last need, so any larger peak reallocates) and is left alone by the third."""
    first = call(False)
    w1 = stat()
    call(True)
    w2 = stat()
    third = call(False)
    w3 = stat()
    print(f"side_workspace_bytes: {w1} -> {w2} -> {w3}")
    assert w2 > w1 and w3 == w2
    for a, b in zip(first, third):
        np.testing.assert_array_equal(a, b)


def test_hed_grow_and_return():
    e = make_engine()     # its own engine: the workspace has to start below the large call's need
    try:
        small, large = pictures((1, 3, 32, 48), 1), pictures((2, 3, 64, 64), 2)
        grow_and_return(lambda big: (e.hed(large if big else small),), lambda: e.stat("side_workspace_bytes"))
    finally:
        e.close()


def test_sd3_text_encoder_grow_and_return():
    """An integer source and two destinations: token ids in, hidden states and pooled output back."""
    e = make_engine3()
    try:
        ids = np.random.default_rng(5).integers(0, TCFG.clip_l.vocab, (4, 77)).astype(np.int32)
        grow_and_return(lambda big: e.text_encoder("clip_l", ids if big else ids[:1].copy()), lambda: e.base.stat("side_workspace_bytes"))
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ captured loops and a regrow
def test_captured_loops_survive_a_regrow():
    e = make_engine()
    try:
        kw = sample_kw()
        e.set_option("graph", 1)
        c0, r0 = e.stat("graph_captures"), e.stat("graph_replays")
        first = e.ddim_sample(**kw)
        again = e.ddim_sample(**kw)
        assert (e.stat("graph_captures"), e.stat("graph_replays")) == (c0 + 1, r0 + 1)
        np.testing.assert_array_equal(again, first)
        w0 = e.stat("side_workspace_bytes")
        edge_big = e.hed(pictures((2, 3, 128, 128), 3))          # larger than anything before: the workspace is reallocated
        assert e.stat("side_workspace_bytes") > w0
        after = e.ddim_sample(**kw)
        assert (e.stat("graph_captures"), e.stat("graph_replays")) == (c0 + 2, r0 + 1)
        np.testing.assert_array_equal(after, first)
        w1 = e.stat("side_workspace_bytes")
        e.hed(pictures((1, 3, 32, 48), 1))                       # fits: nothing is reallocated, the captured loop stays
        assert e.stat("side_workspace_bytes") == w1
        last = e.ddim_sample(**kw)
        assert (e.stat("graph_captures"), e.stat("graph_replays")) == (c0 + 2, r0 + 2)
        np.testing.assert_array_equal(last, first)
        np.testing.assert_array_equal(e.hed(pictures((2, 3, 128, 128), 3)), edge_big)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ host and device callers
# (HED, vae_encode, the SD3 VAE, clip_vision on uint8 pictures and the M-LSD line map compare the two in their own test files)
def same(host, dev):
    host, dev = (host, dev) if isinstance(host, tuple) else ((host,), (dev,))
    assert len(host) == len(dev)
    for h, d in zip(host, dev):
        assert not E._is_torch(h) and d.is_cuda
        np.testing.assert_array_equal(d.cpu().numpy(), h)


def test_host_and_device_callers_agree(eng):
    import torch
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    z = np.random.default_rng(7).standard_normal((2, 4, 8, 8)).astype(np.float32)
    same(eng.vae_decode(z), eng.vae_decode(cuda(z)))
    ids = W.synth_token_ids(W.TINY, 3, seed=11)
    same(eng.text_encode(ids), eng.text_encode(cuda(ids)))
    same(eng.text_encode(ids, clip_skip=1), eng.text_encode(cuda(ids), clip_skip=1))
    pics = np.random.default_rng(8).integers(0, 256, (2, 64, 96, 3)).astype(np.uint8)
    same(eng.mlsd(pics, what="tpmap"), eng.mlsd(cuda(pics), what="tpmap"))
    same(eng.mlsd(pics, 0.0, 0.0, what="segments"), eng.mlsd(cuda(pics), 0.0, 0.0, what="segments"))
    pv = np.random.default_rng(9).standard_normal((2, 3, TOWER.image_size, TOWER.image_size)).astype(np.float32)
    names = ("embeds", "pooled", "hidden")
    same(eng.clip_vision(pv, names, prefix=TOWER.prefix), eng.clip_vision(cuda(pv), names, prefix=TOWER.prefix))
    emb = eng.clip_vision(pv, "embeds", prefix=TOWER.prefix)
    fh, sh = eng.safety_check(emb, return_scores=True)          # (both come back as NumPy)
    fd, sdv = eng.safety_check(cuda(emb), return_scores=True)
    np.testing.assert_array_equal(fd, fh)
    np.testing.assert_array_equal(sdv, sh)


def test_sd3_text_host_and_device_callers_agree(eng3):
    import torch
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    g = np.random.default_rng(12)
    il = g.integers(0, TCFG.clip_l.vocab, (2, 77)).astype(np.int32)
    ig = g.integers(0, TCFG.clip_g.vocab, (2, 77)).astype(np.int32)
    it = g.integers(0, TCFG.t5.vocab, (2, 20)).astype(np.int32)
    same(eng3.text_encoder("clip_l", il, clip_skip=1), eng3.text_encoder("clip_l", cuda(il), clip_skip=1))
    same(eng3.text_encoder("clip_g", ig), eng3.text_encoder("clip_g", cuda(ig)))
    same(eng3.text_encoder("t5", it), eng3.text_encoder("t5", cuda(it)))
    same(eng3.encode_prompt_ids(il, ig, it), eng3.encode_prompt_ids(cuda(il), cuda(ig), cuda(it)))


# ------------------------------------------------------------------------------------------------ a refused call
def test_a_refused_call_leaves_the_engine_whole(eng):
    fresh = make_engine()
    try:
        kw, x = sample_kw(), pictures((1, 3, 32, 48), 1)
        want_lat, want_edge = fresh.ddim_sample(**kw), fresh.hed(x)
    finally:
        fresh.close()
    with pytest.raises(E.PdError, match="multiples of 16"):
        eng.hed(pictures((1, 3, 60, 64), 4))
    np.testing.assert_array_equal(eng.ddim_sample(**kw), want_lat)
    np.testing.assert_array_equal(eng.hed(x), want_edge)
