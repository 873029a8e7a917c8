"""SD3's VAE without a GPU: the parameter inventory against the reference modules' (through the diffusers <-> ldm rename of
tests/sd3_vae_ref.py), the ctypes mirror of pd_sd3_vae_config against what the C side reports, and the pipeline's routing of
the image ends (engine VAE by default, injected callables first, the old errors without either)."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest

from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import sd3
from prompt_diffusion_amd.pipeline_sd3 import StableDiffusion3PromptDiffusionPipeline
from tests import sd3_vae_ref as R


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "sd3_vae.npz"))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(E.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return E.load_library()


def test_spec_matches_reference_inventory(fx):
    """Every tensor of sd3_vae_spec(SD3_MEDIUM_VAE), renamed to ldm, is a tensor of the reference's Encoder / Decoder (z 16, no quant
    convs) with the same shape up to the attention's 1x1 kernel axes -- and the other way round."""
    inv = {n: tuple(s) for n, s in json.loads(str(fx["full_spec"]))}
    cfg = sd3.SD3_MEDIUM_VAE
    nl = len(cfg.ch_mult)
    spec = sd3.sd3_vae_spec(cfg)
    mine = {R.diffusers_to_ldm(n, nl): R.ldm_shape(R.diffusers_to_ldm(n, nl), s) for n, s, _ in spec}
    assert len(mine) == len(spec) == 244
    assert mine == inv
    assert not any("quant_conv" in n for n, _, _ in spec)
    assert dict((n, s) for n, s, _ in spec)["vae.decoder.mid_block.attentions.0.to_q.weight"] == (512, 512)
    dec_only = sd3.sd3_vae_spec(cfg, encoder=False)
    assert all(n.startswith("vae.decoder.") for n, _, _ in dec_only) and len(dec_only) == 138


@pytest.mark.parametrize("cfg", [sd3.SD3_MEDIUM_VAE, sd3.SD3_TINY_VAE, sd3.SD3VaeConfig(ch=32, ch_mult=(1, 2), num_res_blocks=1)])
def test_rename_is_a_bijection(cfg):
    nl = len(cfg.ch_mult)
    names = [n for n, _, _ in sd3.sd3_vae_spec(cfg)]
    ldm = [R.diffusers_to_ldm(n, nl) for n in names]
    assert len(set(ldm)) == len(names)
    assert [R.ldm_to_diffusers(n, nl) for n in ldm] == names
    assert not any("blocks" in n or "to_" in n or "resnets" in n for n in ldm)      # nothing left in diffusers' vocabulary
    # up_blocks count in execution order: the first one is ldm's highest level
    assert R.diffusers_to_ldm("vae.decoder.up_blocks.0.resnets.2.conv1.weight", nl) == f"decoder.up.{nl - 1}.block.2.conv1.weight"


def test_synth_state_dict_follows_spec():
    sd = sd3.synth_sd3_vae_state_dict(sd3.SD3_TINY_VAE)
    assert [(n, a.shape) for n, a in sd.items()] == [(n, tuple(s)) for n, s, _ in sd3.sd3_vae_spec(sd3.SD3_TINY_VAE)]
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in sd.values())


def test_config_struct_matches_library(lib):
    size, off_scale, off_shift = C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.pd_sd3_vae_config_layout(C.byref(size), C.byref(off_scale), C.byref(off_shift)) == 0
    S = sd3.pd_sd3_vae_config
    assert C.sizeof(S) == size.value
    assert S.scaling_factor.offset == off_scale.value and S.shift_factor.offset == off_shift.value
    order = [n for n, _ in S._fields_]
    assert order == ["ch", "num_levels", "ch_mult", "num_res_blocks", "z_channels", "out_ch", "encoder", "quant_conv", "post_quant_conv",
                     "scaling_factor", "shift_factor"]
    assert S.ch_mult.size == 4 * E.PD_MAX_LEVELS and S.num_res_blocks.offset == 8 + 4 * E.PD_MAX_LEVELS
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pdengine.h")).read()
    body = hdr[hdr.index("typedef struct pd_sd3_vae_config"):hdr.index("} pd_sd3_vae_config;")]
    pos = [body.index(n) for n in ("ch,", "num_levels", "ch_mult[", "num_res_blocks", "z_channels", "out_ch", "encoder", " quant_conv",
                                   "post_quant_conv", "scaling_factor", "shift_factor")]
    assert pos == sorted(pos)
    for n in ("pd_sd3_vae_configure", "pd_sd3_vae_weights_missing", "pd_sd3_vae_decode", "pd_sd3_vae_encode", "pd_op_vae_attention"):
        assert n in E.EXPORTS and hasattr(lib, n)


# ---------------------------------------------------------------------------------------------------- pipeline routing
class StubEngine:
    """Records what the pipeline asks of an engine; its 'VAE' is arithmetic that shows whether shift / scaling were applied once."""

    def __init__(self, vae=True, encoder=True):
        self.cfg = types.SimpleNamespace(in_channels=16, force_zeros_for_pooled_projection=False, joint_dim=8, pooled_dim=4)
        self.vae_cfg = sd3.SD3VaeConfig(scaling_factor=2.0, shift_factor=0.25) if vae else None
        self.vae_has_encoder = vae and encoder
        self.text_cfg = None
        self.calls = []

    def vae_encode(self, images, mode="sample", noise=None, raw=False):
        self.calls.append(("vae_encode", mode, raw, tuple(images.shape)))
        x = np.asarray(images, np.float32)
        return np.repeat(x.mean(1, keepdims=True), 16, 1)[:, :, ::8, ::8].copy()       # "latents" = the mean colour, raw

    def vae_decode(self, latents, raw=False):
        self.calls.append(("vae_decode", raw, tuple(latents.shape)))
        z = np.asarray(latents, np.float32)
        return np.repeat(np.repeat(z[:, :3], 8, 2), 8, 3)

    def down_proj(self, cond, gt):
        self.calls.append(("down_proj", tuple(cond.shape)))
        return 0.5 * (np.asarray(cond) + np.asarray(gt))

    def encode_support_pair(self, cond, gt, vae=None):
        self.calls.append(("encode_support_pair", tuple(cond.shape)))
        return self.vae_encode(self.down_proj(cond, gt), mode="sample", raw=True)

    def sample(self, latents, pe, ppe, npe, nppe, control_latents=None, pair_latents=None, **kw):
        self.calls.append(("sample", tuple(latents.shape)))
        self.seen = dict(control=control_latents, pair=pair_latents)
        return np.asarray(latents, np.float32)


def _call(pipe, control_image, pair, output_type="np", **kw):
    B = 1
    pe, ppe = np.zeros((B, 4, 8), np.float32), np.zeros((B, 4), np.float32)
    lat = np.full((B, 16, 2, 2), 0.5, np.float32)
    return pipe(prompt_embeds=pe, pooled_prompt_embeds=ppe, negative_prompt_embeds=pe, negative_pooled_prompt_embeds=ppe, control_image=control_image,
                control_image_pair=pair, latents=lat, num_inference_steps=2, output_type=output_type, **kw)


IMG = np.full((1, 3, 16, 16), 0.75, np.float32)        # [0, 1] image: prepare_image maps it to 0.5
PAIR = [np.full((1, 3, 16, 16), 1.0, np.float32), np.full((1, 3, 16, 16), 0.5, np.float32)]   # -> 1.0 and 0.0, projected to 0.5


def test_pipeline_uses_engine_vae_once_with_the_right_scaling():
    eng = StubEngine()
    pipe = StableDiffusion3PromptDiffusionPipeline(eng)
    assert pipe.vae_scaling_factor == 2.0 and pipe.vae_shift_factor == 0.25     # from the engine's VAE config
    out = _call(pipe, IMG, PAIR)["images"]
    names = [c[0] for c in eng.calls]
    # pair: encode_support_pair (down_proj + one raw encode); control image: one raw encode; one raw decode
    assert names == ["encode_support_pair", "down_proj", "vae_encode", "vae_encode", "sample", "vae_decode"]
    assert all(c[2] is True for c in eng.calls if c[0] == "vae_encode") and [c for c in eng.calls if c[0] == "vae_decode"][0][1] is True
    # (0.5 - 0.25) * 2 = 0.5 for both conditions: shift and scaling applied exactly once
    np.testing.assert_allclose(eng.seen["control"], 0.5, rtol=0, atol=1e-6)
    np.testing.assert_allclose(eng.seen["pair"], 0.5, rtol=0, atol=1e-6)
    assert eng.seen["control"].shape == (1, 16, 2, 2)
    # decode saw 0.5 / 2 + 0.25 = 0.5; the image is clip(0.5 / 2 + 0.5) = 0.75, NHWC for "np"
    assert out.shape == (1, 16, 16, 3)
    np.testing.assert_allclose(out, 0.75, rtol=0, atol=1e-6)
    assert _call(pipe, IMG, PAIR, output_type="pt")["images"].shape == (1, 3, 16, 16)
    pil = _call(pipe, IMG, PAIR, output_type="pil")["images"]
    assert len(pil) == 1 and pil[0].size == (16, 16) and pil[0].getpixel((0, 0)) == (191, 191, 191)
    # PIL images and uint8 arrays are [0, 1] images too (191 / 255 = 0.749 -> 2 x - 1 = 0.498 -> (0.498 - 0.25) * 2)
    from PIL import Image
    gray = Image.new("RGB", (16, 16), (191, 191, 191))
    _call(pipe, gray, [Image.new("RGB", (16, 16), (255, 255, 255)), np.full((16, 16, 3), 128, np.uint8)], output_type="latent")
    np.testing.assert_allclose(eng.seen["control"], (2 * 191 / 255 - 1 - 0.25) * 2, rtol=0, atol=1e-5)
    np.testing.assert_allclose(eng.seen["pair"], (0.5 * (1.0 + 2 * 128 / 255 - 1) - 0.25) * 2, rtol=0, atol=1e-5)
    # explicit factors win over the engine's
    assert StableDiffusion3PromptDiffusionPipeline(eng, vae_scaling_factor=1.5, vae_shift_factor=0.06).vae_scaling_factor == 1.5


def test_injected_callables_keep_precedence():
    eng = StubEngine()
    seen = []
    pipe = StableDiffusion3PromptDiffusionPipeline(
        eng, vae_encode=lambda x: (seen.append("enc"), np.full((x.shape[0], 16, 2, 2), 1.25, np.float32))[1],
        vae_decode=lambda z: (seen.append("dec"), np.zeros((z.shape[0], 3, 16, 16), np.float32))[1],
        down_proj=lambda p: (seen.append("proj"), p[:, :3])[1])
    out = _call(pipe, IMG, PAIR)["images"]
    assert seen == ["proj", "enc", "enc", "dec"]
    assert [c[0] for c in eng.calls] == ["sample"]                     # the engine's VAE was not touched
    np.testing.assert_allclose(eng.seen["control"], (1.25 - 0.25) * 2.0, rtol=0, atol=1e-6)
    np.testing.assert_allclose(out, 0.5, rtol=0, atol=1e-6)
    # an injected encoder with the engine's projection
    eng2 = StubEngine()
    pipe2 = StableDiffusion3PromptDiffusionPipeline(eng2, vae_encode=lambda x: np.full((x.shape[0], 16, 2, 2), 1.25, np.float32))
    _call(pipe2, IMG, PAIR, output_type="latent")
    assert [c[0] for c in eng2.calls] == ["down_proj", "sample"]


def test_old_errors_without_a_vae():
    eng = StubEngine(vae=False)
    pipe = StableDiffusion3PromptDiffusionPipeline(eng)
    assert pipe.vae_scaling_factor == 1.5305 and pipe.vae_shift_factor == 0.0609
    lat = np.zeros((1, 16, 2, 2), np.float32)
    with pytest.raises(ValueError, match="unless the pipeline was given `vae_encode`"):
        _call(pipe, IMG, lat)
    with pytest.raises(ValueError, match="image pairs need `vae_encode` and `down_proj`"):
        _call(pipe, lat, PAIR)
    with pytest.raises(ValueError, match="needs the `vae_decode` callable"):
        _call(pipe, lat, lat)
    assert _call(pipe, lat, lat, output_type="latent")["images"].shape == (1, 16, 2, 2)
    # a decoder-only engine VAE decodes but does not encode
    dec_only = StableDiffusion3PromptDiffusionPipeline(StubEngine(encoder=False))
    assert _call(dec_only, lat, lat)["images"].shape == (1, 16, 16, 3)
    with pytest.raises(ValueError, match="unless the pipeline was given `vae_encode`"):
        _call(dec_only, IMG, lat)
