"""IP-Adapter on the CPU: the kernel bound of tests/ip_adapter_ref.py has teeth on the inputs the GPU test uses, the checkpoint parser,
the pipelines' argument handling on a stub engine, and the effect size of the seeded TINY adapter in the NumPy restatement (so that the
GPU tests cannot pass with the adapter silently off)."""
import functools

import numpy as np
import pytest

from oracle import pd_oracle as O
from prompt_diffusion_amd import ip_adapter as IP
from prompt_diffusion_amd import weights as W
from prompt_diffusion_amd.pipeline import PromptDiffusionImg2ImgPipeline, PromptDiffusionInpaintPipeline, PromptDiffusionPipeline
from tests import attn_ref as R
from tests import ip_adapter_ref as IR

# (B, N, C, heads, T, Bk): the kernel shapes of the GPU test -- every head dim 8 .. 160 the engine serves is C / heads of one of them
KERNEL_SHAPES = [(2, 100, 320, 8, 4, 2), (1, 64, 1280, 8, 16, 1), (2, 48, 64, 8, 4, 2), (1, 1024, 640, 8, 1, 1), (2, 12, 128, 8, 5, 2),
                 (3, 100, 320, 8, 4, 1), (1, 33, 320, 8, 64, 1),
                 (1, 16, 1280, 8, 64, 1)]      # dh 160 with 64 keys: in fp32 storage they pass through LDS 32 at a time

KERNEL_FAMILIES = ("normal", "negative", "peaked_last", "large")
KERNEL_SCALES = (1.0, -0.5)
MODES = ("f32", "f16x2", "f16", "bf16")
# the seeded adapter of the TINY tests: 4 tokens from a 64-wide embedding (the proj_dim of the tiny image tower), to_k_ip / to_v_ip at
# twice the recipe's standard deviation
TINY_T, TINY_E, TINY_GAIN, TINY_SEED = 4, 64, 2.0, 4321


def kernel_seed(family, shape):
    B, N, C, heads, T, Bk = shape
    return 1000 * R.FAMILIES.index(family) + 97 * B + 13 * N + 7 * T + 3 * heads + C + 31 * Bk


@functools.lru_cache(maxsize=None)
def kernel_case(mode, family, shape, s):
    """(q, att, k, v, ref, bound) of one case, shared and read-only"""
    B, N, C, heads, T, Bk = shape
    q, att, k, v = IR.make_kernel_inputs(family, kernel_seed(family, shape), B, N, C, heads, T, mode, Bk)
    ref, _ = IR.ip_attn_add_ref(q, att, k, v, heads, s)
    bound = IR.ip_attn_add_bound(mode, q, att, k, v, heads, s)
    for a in (q, att, k, v, ref, bound):
        a.setflags(write=False)
    return q, att, k, v, ref, bound


def tiny_adapter():
    return IP.synth_ip_adapter(W.TINY, TINY_T, TINY_E, TINY_SEED, TINY_GAIN)


def tiny_embeds(Bi, seed=77):
    g = np.random.default_rng(seed)
    return g.standard_normal((Bi, TINY_E)).astype(np.float32), (0.5 * g.standard_normal((Bi, TINY_E))).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the bound has teeth
def _applies(mutant, mode, shape, s):
    """where a mutant computes something else than the kernel: one key has softmax 1 whatever its logit (T = 1: next head's keys and
    the scale inside the softmax change nothing); s = 1 inside the softmax is the kernel itself; rounding o to an fp32 storage type is
    no rounding; samples can only be swapped where each has keys of its own"""
    B, N, C, heads, T, Bk = shape
    if mutant in ("k_next_head", "scale_in_softmax") and T == 1:
        return False
    if mutant == "scale_in_softmax" and s == 1.0:
        return False
    if mutant == "round_o" and (R.STORAGE[mode] == "f32" or T == 1):      # (T = 1: o is the one value row, already a value of T)
        return False
    if mutant == "swap_samples" and (B < 2 or Bk != B):
        return False
    return True


@pytest.mark.parametrize("mode", MODES)
def test_reference_is_inside_and_every_mutant_outside_the_bound(mode):
    """the reference rounded to the storage type passes; each mutant exceeds the bound somewhere in every (shape, s) it applies to, on the
    family that shows it (a peaked last key for the dropped key, any family for the others)"""
    seen = set()
    for shape in KERNEL_SHAPES:
        B, N, C, heads, T, Bk = shape
        for s in KERNEL_SCALES:
            for mutant in IR.KERNEL_MUTANTS:
                if not _applies(mutant, mode, shape, s):
                    continue
                worst = 0.0
                for family in KERNEL_FAMILIES:
                    q, att, k, v, ref, bound = kernel_case(mode, family, shape, s)
                    if mutant == IR.KERNEL_MUTANTS[0]:
                        own = R.round_like(ref.astype(np.float32), mode)
                        assert R.check(own, ref, bound)[0] <= 1.0, (mode, family, shape, s)
                    with np.errstate(invalid="ignore"):      # (the dropped key of T = 1 leaves an empty softmax: NaN, infinitely wrong)
                        got, _ = IR.ip_attn_add_ref(q, att, k, v, heads, s, mode=mode, mutant=mutant)
                    worst = max(worst, R.check(got, ref, bound)[0])
                assert worst > 1.0, f"{mode} {shape} s={s}: mutant {mutant} stays inside the bound (worst err / bound {worst:.3f})"
                seen.add(mutant)
    assert seen == set(IR.KERNEL_MUTANTS) - ({"round_o"} if R.STORAGE[mode] == "f32" else set()), seen


# ------------------------------------------------------------------------------------------------ parser
def test_parser_accepts_both_layouts_and_orders_the_blocks():
    sd = IP.synth_ip_adapter(W.SD15, 4, 1024, seed=3)
    T, E, flat = IP.parse_ip_adapter(sd)
    assert (T, E) == (4, 1024) and set(flat) == set(sd)
    T2, E2, nest = IP.parse_ip_adapter(IP.nested(sd))
    assert (T2, E2) == (4, 1024) and set(nest) == set(sd)
    for k in sd:
        np.testing.assert_array_equal(nest[k], sd[k])
    # id -> block: six blocks of the input side, nine of the output side, the middle block last (id 31)
    widths = IP.block_widths(W.SD15)
    assert widths == [320, 320, 640, 640, 1280, 1280] + [1280] * 3 + [640] * 3 + [320] * 3 + [1280]
    pre = IP.block_prefixes(W.SD15)
    assert pre[0] == W.UNET_PREFIX + "input_blocks.1.1." and pre[5] == W.UNET_PREFIX + "input_blocks.8.1."
    assert pre[6] == W.UNET_PREFIX + "output_blocks.3.1." and pre[14] == W.UNET_PREFIX + "output_blocks.11.1."
    assert pre[15] == W.UNET_PREFIX + "middle_block.1."
    for j, c in enumerate(widths):
        assert flat[f"ip_adapter.{2 * j + 1}.to_k_ip.weight"].shape == (c, 768)
    assert "ip_adapter.31.to_v_ip.weight" in flat and "ip_adapter.33.to_k_ip.weight" not in flat
    # the reduced network has the same 16 blocks
    assert len(IP.block_widths(W.TINY)) == 16 and IP.parse_ip_adapter(tiny_adapter(), W.TINY)[:2] == (TINY_T, TINY_E)


def test_parser_reads_bin(tmp_path):
    sd = tiny_adapter()
    import torch
    p = tmp_path / "ip.bin"
    torch.save({k: {k2: torch.from_numpy(v2) for k2, v2 in v.items()} for k, v in IP.nested(sd).items()}, str(p))
    T, E, got = IP.parse_ip_adapter(str(p), W.TINY)
    assert (T, E) == (TINY_T, TINY_E)
    np.testing.assert_array_equal(got["ip_adapter.31.to_k_ip.weight"], sd["ip_adapter.31.to_k_ip.weight"])


def test_parser_reads_safetensors(tmp_path):
    save_file = pytest.importorskip("safetensors.numpy").save_file
    sd = tiny_adapter()
    p = tmp_path / "ip.safetensors"
    save_file(sd, str(p))
    T, E, got = IP.parse_ip_adapter(str(p), W.TINY)
    assert (T, E) == (TINY_T, TINY_E)
    np.testing.assert_array_equal(got["image_proj.proj.weight"], sd["image_proj.proj.weight"])


@pytest.mark.parametrize("key,shape", [
    ("image_proj.latents", (1, 16, 768)),                                   # Resampler ("plus")
    ("image_proj.layers.0.0.to_q.weight", (768, 768)),
    ("image_proj.proj.0.weight", (1024, 1024)),                             # full-face MLP
    ("ip_adapter.1.to_k_lora.down.weight", (128, 320)),                     # FaceID
    ("ip_adapter.33.to_k_ip.weight", (640, 2048)),                          # an SDXL id
    ("something.else", (3,)),
])
def test_parser_refuses_other_layouts_and_names_the_key(key, shape):
    sd = IP.synth_ip_adapter(W.SD15, 4, 1024, seed=3)
    sd[key] = np.zeros(shape, np.float32)
    with pytest.raises(NotImplementedError, match=key.replace(".", r"\.")):
        IP.parse_ip_adapter(sd)


def test_parser_refuses_sdxl_widths_missing_tensors_and_several_adapters():
    sd = IP.synth_ip_adapter(W.SD15, 4, 1024, seed=3)
    wide = dict(sd)
    wide["ip_adapter.1.to_k_ip.weight"] = np.zeros((640, 2048), np.float32)
    with pytest.raises(NotImplementedError, match=r"ip_adapter\.1\.to_k_ip\.weight"):
        IP.parse_ip_adapter(wide)
    wide = dict(sd)
    wide["image_proj.proj.weight"] = np.zeros((4 * 2048 + 8, 1280), np.float32)
    with pytest.raises(NotImplementedError, match=r"image_proj\.proj\.weight"):
        IP.parse_ip_adapter(wide)
    less = {k: v for k, v in sd.items() if k != "ip_adapter.7.to_v_ip.weight"}
    with pytest.raises(NotImplementedError, match=r"ip_adapter\.7\.to_v_ip\.weight"):
        IP.parse_ip_adapter(less)
    with pytest.raises(NotImplementedError, match="2 IP-Adapters"):
        IP.parse_ip_adapter([sd, sd])


# ------------------------------------------------------------------------------------------------ pipeline arguments on a stub engine
class _Boom(Exception):
    pass


class _StubEngine:
    """Records the adapter calls; anything else the call body asks of the engine ends the call with _Boom."""
    cfg = W.TINY

    def __init__(self):
        self.log = []
        self.loaded = {}

    def configure_ip_adapter(self, T, E):
        self.log.append(("configure", T, E))

    def load_state_dict(self, sd, strict=True):
        self.loaded = dict(sd)

    def ip_adapter_weights_missing(self):
        return 0

    def ip_adapter_set_scale(self, s):
        self.log.append(("scale", s))

    def ip_adapter_set_image(self, emb, neg=None):
        self.log.append(("set", np.array(emb), None if neg is None else np.array(neg)))

    def ip_adapter_clear_image(self):
        self.log.append(("clear",))

    def __getattr__(self, name):
        raise _Boom(name)


def _call_kw(B=1, hw=64):
    img = np.zeros((B, hw, hw, 3), np.float32)
    emb = np.zeros((B, 77, 96), np.float32)
    return dict(prompt_embeds=emb, negative_prompt_embeds=emb, image=img, image_pair=[img.copy(), img.copy()])


@pytest.fixture(params=[PromptDiffusionPipeline, PromptDiffusionImg2ImgPipeline, PromptDiffusionInpaintPipeline])
def loaded(request):
    eng = _StubEngine()
    pipe = request.param(eng)
    pipe.load_ip_adapter(IP.nested(tiny_adapter()))
    assert eng.log[0] == ("configure", TINY_T, TINY_E) and len(eng.loaded) == 4 + 32 and eng.log[1] == ("scale", 1.0)
    del eng.log[:]
    if request.param is PromptDiffusionPipeline:
        kw = _call_kw
    else:       # `image` is the init image there (given as its latents), `control_image` the query
        lat = lambda B: np.zeros((B, 4, 8, 8), np.float32)
        if request.param is PromptDiffusionImg2ImgPipeline:
            kw = lambda B=1: dict(_call_kw(B), control_image=_call_kw(B)["image"], image=lat(B))
        else:
            kw = lambda B=1: dict(_call_kw(B), control_image=_call_kw(B)["image"], image=lat(B), mask_image=np.zeros((B, 64, 64), np.float32))
    return pipe, eng, kw


def _sets(eng):
    return [e for e in eng.log if e[0] == "set"]


def test_without_an_adapter_both_arguments_keep_raising():
    pipe = PromptDiffusionPipeline(_StubEngine())
    for arg in ("ip_adapter_image", "ip_adapter_image_embeds"):
        with pytest.raises(NotImplementedError, match="ip_adapter_image"):
            pipe(**{arg: np.zeros((1, TINY_E), np.float32)}, **_call_kw())
    assert pipe.engine.log == []
    with pytest.raises(ValueError, match="load_ip_adapter"):
        pipe.set_ip_adapter_scale(0.5)


def test_embeds_shapes_split_broadcast_and_clear_after_an_exception(loaded):
    pipe, eng, kw = loaded
    e1 = np.arange(TINY_E, dtype=np.float32)[None]
    # [B, E], [B, 1, E] and one-element lists of either; the body then fails on the stub, and the image is cleared all the same
    for emb in (e1, e1[:, None], [e1], [e1[:, None]]):
        del eng.log[:]
        with pytest.raises(_Boom):
            pipe(ip_adapter_image_embeds=emb, **kw())
        assert [e[0] for e in eng.log] == ["set", "clear"]
        np.testing.assert_array_equal(eng.log[0][1], e1)
        assert eng.log[0][2] is None
    # 2 B rows under guidance: [negative ; positive]
    del eng.log[:]
    both = np.concatenate([-e1, e1])
    with pytest.raises(_Boom):
        pipe(ip_adapter_image_embeds=both, **kw())
    np.testing.assert_array_equal(_sets(eng)[0][1], e1)
    np.testing.assert_array_equal(_sets(eng)[0][2], -e1)
    assert eng.log[-1] == ("clear",)
    # ... without guidance they are two positive rows: for a batch of one, a mismatch that names both numbers
    del eng.log[:]
    with pytest.raises(ValueError, match=r"2 image embeddings .* batch of 1"):
        pipe(ip_adapter_image_embeds=both, guidance_scale=1.0, **kw())
    assert eng.log == []
    # one row for a batch of two prompts x two images each: broadcast (Bi = 1); one row per prompt: repeated per image
    del eng.log[:]
    with pytest.raises(_Boom):
        pipe(ip_adapter_image_embeds=e1, num_images_per_prompt=2, **kw(2))
    assert _sets(eng)[0][1].shape == (1, TINY_E)
    del eng.log[:]
    two = np.stack([e1[0], 2 * e1[0]])
    with pytest.raises(_Boom):
        pipe(ip_adapter_image_embeds=two, num_images_per_prompt=2, **kw(2))
    np.testing.assert_array_equal(_sets(eng)[0][1], np.stack([e1[0], e1[0], 2 * e1[0], 2 * e1[0]]))
    del eng.log[:]
    with pytest.raises(ValueError, match=r"3 image embeddings .* batch of 4"):
        pipe(ip_adapter_image_embeds=np.zeros((3, TINY_E), np.float32), num_images_per_prompt=2, **kw(2))
    # several adapters' worth of embeddings / several images per adapter
    with pytest.raises(NotImplementedError, match="2 entries"):
        pipe(ip_adapter_image_embeds=[e1, e1], **kw())
    with pytest.raises(NotImplementedError, match="more than one image per adapter"):
        pipe(ip_adapter_image_embeds=np.zeros((1, 2, TINY_E), np.float32), **kw())


def test_image_goes_through_encode_image_and_scales_reach_the_engine(loaded):
    pipe, eng, kw = loaded
    seen = []

    class Out:
        def __init__(self, pv):
            self.image_embeds = np.full((pv.shape[0], TINY_E), 3.0, np.float32)

    def encoder(pv, **k):
        seen.append(pv.shape)
        return Out(pv)

    pipe.image_encoder = encoder
    pipe._host_pixel_values = lambda x: np.zeros((1 if not hasattr(x, "shape") or x.ndim == 3 else x.shape[0], 3, 8, 8), np.float32)
    from PIL import Image
    pic = Image.fromarray(np.zeros((20, 24, 3), np.uint8))
    with pytest.raises(_Boom):
        pipe(ip_adapter_image=pic, **kw())
    assert seen and _sets(eng)[0][1].shape == (1, TINY_E) and float(_sets(eng)[0][1][0, 0]) == 3.0
    np.testing.assert_array_equal(_sets(eng)[0][2], np.zeros((1, TINY_E), np.float32))      # encode_image's zeros_like
    assert eng.log[-1] == ("clear",)
    with pytest.raises(NotImplementedError, match="2 entries"):
        pipe(ip_adapter_image=[pic, pic], **kw())
    del eng.log[:]
    pipe.set_ip_adapter_scale(0.25)
    pipe.set_ip_adapter_scale([0.5] * 16)
    assert eng.log == [("scale", 0.25), ("scale", [0.5] * 16)]
    with pytest.raises(NotImplementedError, match="already loaded"):
        pipe.load_ip_adapter(tiny_adapter())
    pipe.unload_ip_adapter()
    with pytest.raises(NotImplementedError, match="ip_adapter_image"):
        pipe(ip_adapter_image=pic, **kw())


# ------------------------------------------------------------------------------------------------ effect size
def test_seeded_tiny_adapter_moves_eps_by_more_than_ten_tolerances():
    """adapter-on eps of the restatement against adapter-off eps, relative to max |eps|: more than 10 x the 1e-4 the f32 GPU test allows,
    under guidance (tokens [unconditional ; conditional]) and for a single block alone"""
    cfg = W.TINY
    sd, lay = W.synth_state_dict(cfg), O.make_layouts(cfg, W)
    ip_sd = tiny_adapter()
    B = 1
    inp = W.synth_inputs(cfg, B, 8, 8)
    x, t = np.concatenate([inp["x_T"]] * 2), np.full((2 * B,), 801, np.int64)
    ctx = np.concatenate([inp["ctx_uncond"], inp["ctx_cond"]])
    pair, qry = np.concatenate([inp["pair"]] * 2), np.concatenate([inp["query"]] * 2)
    off = O.apply_model(sd, cfg, lay, x, t, ctx, pair, qry)
    cond, _ = tiny_embeds(1)
    tok = IR.call_tokens(ip_sd, TINY_T, cond, None, B, True)
    assert tok.shape == (2, TINY_T, cfg.context_dim) and np.abs(tok[0]).max() > 0.1       # the projection of zeros is LayerNorm(bias)
    slots = IR.slots_of(IP.block_prefixes(cfg, prefix=""))
    rel = lambda a: float(np.abs(a - off).max() / np.abs(off).max())
    with IR.ip_active(ip_sd, slots, tok, np.ones(16, np.float32)):
        on = O.apply_model(sd, cfg, lay, x, t, ctx, pair, qry)
    one = np.zeros(16, np.float32); one[15] = 1.0
    with IR.ip_active(ip_sd, slots, tok, one):
        mid = O.apply_model(sd, cfg, lay, x, t, ctx, pair, qry)
    with IR.ip_active(ip_sd, slots, tok, np.zeros(16, np.float32)):
        zero = O.apply_model(sd, cfg, lay, x, t, ctx, pair, qry)
    print(f"[ip] effect of the seeded TINY adapter on eps: all blocks {rel(on):.3e}, middle block alone {rel(mid):.3e}")
    np.testing.assert_array_equal(zero, off)
    assert rel(on) > 10 * 1e-4 and rel(mid) > 10 * 1e-4
    assert O.cross_attention.__module__ == "oracle.pd_oracle"          # the wrapper is gone
