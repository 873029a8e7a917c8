"""Tiled and sliced VAE calls on the GPU (pd_vae_set_tiling / pd_vae_set_slicing, the pipelines' enable_vae_tiling / enable_vae_slicing).

The blend kernel alone is compared byte for byte with the sequential restatement (tests/vae_tiling_ref.py); whole calls are compared with
tests/golden/vae_tiling.npz -- the reference's own Decoder / Encoder run per tile on the CPU and blended by the restatement -- within the
decoder's bounds on max |diff| / max |ref| (f32 1e-4, f16x2 1e-4, f16 4e-3, bf16 3e-2): the blend is a convex combination and adds no
error beyond the tiles' own.  Where the generator found tiled and untiled results more than ten bounds apart, the tiled call must also
NOT be the untiled result."""
import dataclasses
import os

import numpy as np
import pytest

from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import sd3
from prompt_diffusion_amd import weights as W
from prompt_diffusion_amd.pipeline import PromptDiffusionPipeline

from . import vae_tiling_ref as R

pytestmark = pytest.mark.gpu

TOL = {"f32": 1e-4, "f16x2": 1e-4, "f16": 4e-3, "bf16": 3e-2}
TINY_E = dataclasses.replace(W.TINY, vae_encoder=True)
T, F = 16, 0.25   # the golden's tiling
UNTILED_TINY_F32_LAUNCHES = (76, 60)   # (decode [2, 4, 8, 8], encode [2, 3, 64, 64] moments), f32: measured with the library of the commit before


def relerr(a, b):
    return float(np.abs(np.asarray(a, np.float32) - np.asarray(b, np.float32)).max() / (np.abs(b).max() + 1e-30))


def images_from_key(key, shape):   # tests/golden/make_golden_vae_encoder.py
    return np.random.Generator(np.random.Philox(key=[77, int(key)])).uniform(-1.0, 1.0, shape).astype(np.float32)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "vae_tiling.npz"))


def vae_engine(prec, cfg=TINY_E):
    e = E.Engine(cfg, precision=prec)
    for n, a in {**W.synth_vae_state_dict(cfg), **W.synth_vae_encoder_state_dict(cfg)}.items():
        e.load_tensor(n, a)
    assert e.vae_weights_missing() == 0 and e.vae_encoder_weights_missing() == 0
    return e


@pytest.fixture(scope="module")
def tiny_f32():
    e = vae_engine("f32")
    yield e
    e.close()


# ---------------------------------------------------------------------------------------------- the blend kernel alone
# 25 x 26 latent pixels at T 16: rows of 16, 16 and ONE latent pixel, columns of 16, 16 and 2 (narrower than the blend extent of 4)
@pytest.mark.parametrize("nchw", [True, False])
def test_blend_kernel_is_the_sequential_blend_byte_for_byte(tiny_f32, nchw):
    if nchw:   # the decode side: tiles in image pixels, [B, 3, H, W] out of 4-channel NHWC tiles
        p, cpad, cout, be, limit = E.vae_tile_plan(25, 26, T, F, 8), 4, 3, 32, 96
    else:      # the encode side: tiles of moments, 8-channel NHWC in and out
        p, cpad, cout, be, limit = E.vae_tile_plan(200, 208, T, F, 8, encode=True), 8, 8, 4, 12
    assert (p.rows, p.cols) == (3, 3)
    assert p.tiles[-1].th == (8 if nchw else 1) and p.tiles[-1].tw == (16 if nchw else 2) and p.tiles[-1].eh < be
    rng = np.random.default_rng(3)
    tiles = [rng.standard_normal((2, t.th, t.tw, cpad)).astype(np.float32) for t in p.tiles]
    got = tiny_f32.op_vae_tile_blend(tiles, p, cout, nchw=nchw)
    rows = [[t.transpose(0, 3, 1, 2)[:, :cout] for t in tiles[i * p.cols:(i + 1) * p.cols]] for i in range(p.rows)]
    ref = R.assemble(rows, be, limit)
    if not nchw:
        ref = np.ascontiguousarray(ref.transpose(0, 2, 3, 1))
    assert got.shape == ref.shape
    assert got.tobytes() == ref.tobytes()


def test_blend_hook_refuses_an_inconsistent_plan(tiny_f32):
    p = E.vae_tile_plan(25, 26, T, F, 8)
    tiles = [np.zeros((1, t.th, t.tw, 4), np.float32) for t in p.tiles]
    bad = p._replace(tiles=[t._replace(ev=t.th + 1) if i == 4 else t for i, t in enumerate(p.tiles)])
    with pytest.raises(E.PdError, match="inconsistent"):
        tiny_f32.op_vae_tile_blend(tiles, bad, 3)


# ---------------------------------------------------------------------------------------------- sizes that are not tiled
def test_untiled_size_is_untouched_by_the_switch(tiny_f32):
    e = tiny_f32
    z = np.random.default_rng(0).standard_normal((2, 4, 8, 8)).astype(np.float32)
    x = images_from_key(5, (2, 3, 64, 64))
    n0, t0 = e.stat("launches"), e.stat("vae_tiles")
    img0 = e.vae_decode(z)
    nd = e.stat("launches")
    mom0 = e.vae_encode(x, mode="moments")
    n1 = e.stat("launches")
    # the counts of the engine before tiling existed (its library, same calls, same machine type): the split of vae_forward into entry
    # kernel, layers and exit kernel added no launch to the default path
    assert (nd - n0, n1 - nd) == UNTILED_TINY_F32_LAUNCHES
    e.set_vae_tiling(True)                      # T 64: an 8 x 8 latent is not tiled (h <= T), so the call is the existing one
    assert e.vae_tiling == E.VaeTilingState(True, False, 64, 0.25, e.vae_tiling.tile_batch)
    img1, mom1 = e.vae_decode(z), e.vae_encode(x, mode="moments")
    n2 = e.stat("launches")
    e.set_vae_tiling(False)
    assert img1.tobytes() == img0.tobytes() and mom1.tobytes() == mom0.tobytes()
    assert n2 - n1 == n1 - n0 and e.stat("vae_tiles") == t0


# ---------------------------------------------------------------------------------------------- against the golden
@pytest.mark.parametrize("prec", ["f32", "f16x2", "f16", "bf16"])
def test_tiled_decode_and_encode_match_the_reference_tiles(fx, prec):
    """decode: 32 x 20 latent, 3 x 2 tiles of 16, 16, 8 by 16, 8; encode: 256 x 160 image, tiles of 128, 128, 64 by 128, 64 pixels.
    Fails without the feature: the untiled call is 0.23 (decode) / 0.32 (encode) away from these."""
    e = vae_engine(prec)
    e.set_vae_tiling(True, tile_latent=T, overlap_factor=F)
    img = e.vae_decode(fx["dec_z"])
    assert img.shape == fx["dec_tiled"].shape
    err, away = relerr(img, fx["dec_tiled"]), relerr(img, fx["dec_untiled"])
    print(f"decode {prec}: tiled relerr {err:.3e}, from the untiled golden {away:.3e}")
    x = images_from_key(fx["enc_key"], (1, 3, 256, 160))
    mom = e.vae_encode(x, mode="moments")
    assert mom.shape == fx["enc_tiled"].shape
    err_e, away_e = relerr(mom, fx["enc_tiled"]), relerr(mom, fx["enc_untiled"])
    print(f"encode {prec}: tiled relerr {err_e:.3e}, from the untiled golden {away_e:.3e}")
    assert e.stat("vae_tiles") == 12
    e.close()
    assert err < TOL[prec] and err_e < TOL[prec]
    if prec in fx["dec_differs"]:
        assert away > TOL[prec]
    if prec in fx["enc_differs"]:
        assert away_e > TOL[prec]


def test_tile_batch_one_and_default_agree(fx):
    e = vae_engine("f16")
    e.set_vae_tiling(True, tile_latent=T, overlap_factor=F)           # default tile_batch
    a = e.vae_decode(fx["dec_z"])
    e.set_vae_tiling(True, tile_latent=T, overlap_factor=F, tile_batch=1)
    assert e.vae_tiling.tile_batch == 1
    b = e.vae_decode(fx["dec_z"])
    e.close()
    assert relerr(a, fx["dec_tiled"]) < TOL["f16"] and relerr(b, fx["dec_tiled"]) < TOL["f16"]
    assert relerr(a, b) < TOL["f16"]


def test_fp32_tile_that_cannot_materialise_its_scores_is_named(tiny_f32):
    e = tiny_f32
    e.set_vae_tiling(True, tile_latent=T, overlap_factor=F)
    try:
        with pytest.raises(E.PdError, match=r"tile at \(12, 12\) is 5 x 5 latent pixels"):   # 16 x 5 = 80 tokens still materialises
            e.vae_decode(np.zeros((1, 4, 17, 17), np.float32))
        with pytest.raises(E.PdError, match="overlap_factor"):
            e.set_vae_tiling(True, overlap_factor=0.5)
        assert e.vae_tiling.overlap_factor == F                       # a refused call leaves the state
    finally:
        e.set_vae_tiling(False)
    assert e.vae_tiling[:4] == (False, False, T, F)                   # switching off keeps the parameters ...
    e.set_vae_tiling(True)
    assert e.vae_tiling[:4] == (True, False, 64, 0.25)                # ... switching on replaces them, None: the defaults
    e.set_vae_tiling(False)


def test_thin_remainder_tiles_run_through_the_layers():
    """25 x 17 latent at T 16: rows of 16, 13 (truncated) and ONE latent pixel, columns of 16 and 5 -- tiles of 1 x 16, 13 x 16 and 16 x 5
    through the convs, GroupNorm and the upsamples, and 13 x 5 and 1 x 5 (65 and five tokens, no multiples of 8) through the flash
    attention kernel, which this VAE takes for no other call.
    f16 against the NumPy oracle's decoder per window, blended by the restatement; the decoder's f16 bound."""
    from oracle import pd_oracle as O
    cfg = W.TINY
    vsd = W.synth_vae_state_dict(cfg)
    z = np.random.default_rng(8).standard_normal((1, 4, 25, 17)).astype(np.float32)
    ref = R.tiled_decode(z, T, F, lambda t: O.vae_decode(vsd, cfg, W.vae_layout(cfg), np.ascontiguousarray(t)))   # 1 / scale_factor per element
    e = vae_engine("f16")
    e.set_vae_tiling(True, tile_latent=T, overlap_factor=F)
    assert [(t.h, t.w) for t in e.vae_tile_plan(25, 17).tiles] == [(16, 16), (16, 5), (13, 16), (13, 5), (1, 16), (1, 5)]
    f0 = e.stat("vae_flash_launches")
    got = e.vae_decode(z)
    flash = e.stat("vae_flash_launches") - f0
    e.close()
    assert got.shape == ref.shape == (1, 3, 200, 136)
    err = relerr(got, ref)
    print(f"tiny f16 25x17: relerr {err:.3e}, flash launches {flash}")
    assert flash == 2 and np.isfinite(got).all() and err < TOL["f16"]


# ---------------------------------------------------------------------------------------------- real shapes and dispatch
def test_sd15_shapes_f16_against_the_engines_own_windows():
    """SD1.5's VAE, latent 72 x 64 at the default T 64: tiles of 64 x 64, 64 x 16, 24 x 64 and 24 x 16 on the kernels the full-size
    decoder dispatches, against the restatement applied to the engine's own untiled decodes of the same windows."""
    e = E.Engine(W.SD15, precision="f16")
    e.init_random_weights(7)
    z = (np.random.default_rng(1).standard_normal((1, 4, 72, 64)) * W.SD15.scale_factor).astype(np.float32)
    ref = R.tiled_decode(z, 64, 0.25, lambda t: e.vae_decode(np.ascontiguousarray(t)))
    e.set_vae_tiling(True)
    assert [(t.h, t.w) for t in e.vae_tile_plan(72, 64).tiles] == [(64, 64), (64, 16), (24, 64), (24, 16)]
    got = e.vae_decode(z)
    e.close()
    assert got.shape == ref.shape == (1, 3, 576, 512)
    err = relerr(got, ref)
    print(f"sd15 f16 72x64: relerr {err:.3e}")
    assert np.isfinite(got).all() and err < TOL["f16"]


def test_sd3_tiny_vae_f16_against_the_engines_own_windows():
    net = sd3.SD3Config(in_channels=16, out_channels=16, heads=2, head_dim=64, layers=2, cn_layers=1, joint_dim=96, pooled_dim=40,
                        pos_embed_max_size=12)
    e = sd3.SD3Engine(net, precision="f16")
    e.configure_vae(sd3.SD3_TINY_VAE)
    e.load_state_dict(sd3.synth_sd3_vae_state_dict(sd3.SD3_TINY_VAE), strict=False)
    assert e.vae_tiling == E.VaeTilingState(False, False, 128, 0.25, e.vae_tiling.tile_batch)
    z = np.random.default_rng(2).standard_normal((1, 16, 28, 20)).astype(np.float32)
    x = images_from_key(9, (1, 3, 224, 160))
    ref = R.tiled_decode(z, T, F, lambda t: e.vae_decode(np.ascontiguousarray(t)))             # shift and scaling per element: any window
    ref_m = R.tiled_encode(x, T, F, lambda t: e.vae_encode(np.ascontiguousarray(t), mode="moments"))
    e.set_vae_tiling(True, tile_latent=T, overlap_factor=F)
    assert (e.vae_tile_plan(28, 20).rows, e.vae_tile_plan(28, 20).cols) == (3, 2)
    got, got_m = e.vae_decode(z), e.vae_encode(x, mode="moments")
    e.close()
    assert got.shape == ref.shape and got_m.shape == ref_m.shape
    print(f"sd3 tiny f16: decode relerr {relerr(got, ref):.3e}, moments {relerr(got_m, ref_m):.3e}")
    assert relerr(got, ref) < TOL["f16"] and relerr(got_m, ref_m) < TOL["f16"]


# ---------------------------------------------------------------------------------------------- slicing
def test_sliced_calls_match_unsliced(tiny_f32, fx):
    e = tiny_f32
    rng = np.random.default_rng(4)
    z = rng.standard_normal((3, 4, 8, 8)).astype(np.float32)
    x = images_from_key(6, (3, 3, 64, 64))
    noise = rng.standard_normal((3, 4, 8, 8)).astype(np.float32)
    img0, lat0 = e.vae_decode(z), e.vae_encode(x, mode="sample", noise=noise)
    e.set_vae_slicing(True)
    try:
        assert e.vae_tiling.slicing and not e.vae_tiling.tiling
        img1, lat1 = e.vae_decode(z), e.vae_encode(x, mode="sample", noise=noise)
        # ... and with both switches on each slice is tiled: three times the golden's sample
        e.set_vae_tiling(True, tile_latent=T, overlap_factor=F)
        both = e.vae_decode(np.concatenate([fx["dec_z"]] * 3))
    finally:
        e.set_vae_slicing(False)
        e.set_vae_tiling(False)
    assert img1.shape == img0.shape == (3, 3, 64, 64) and lat1.shape == lat0.shape == (3, 4, 8, 8)
    assert relerr(img1, img0) < TOL["f32"] and relerr(lat1, lat0) < TOL["f32"]
    assert both.shape == (3, 3, 256, 160)
    for b in range(3):
        assert relerr(both[b:b + 1], fx["dec_tiled"]) < TOL["f32"]


# ---------------------------------------------------------------------------------------------- the pipeline
def test_pipeline_switches_reach_the_decode():
    cfg = W.TINY
    e = E.Engine(cfg, precision="f32")
    e.load_state_dict({**W.synth_state_dict(cfg), **W.synth_vae_state_dict(cfg)})
    hw = 128                                                          # a 16 x 16 latent: tiled at T 8 (tiles of 8, 8, 4 per side)
    inp = W.synth_inputs(cfg, 1, hw // 8, hw // 8, seed=5, unit_range=True)
    a, b = inp["pair"][:, :3], inp["pair"][:, 3:]
    kw = dict(prompt_embeds=inp["ctx_cond"], negative_prompt_embeds=inp["ctx_uncond"], image=inp["query"].transpose(0, 2, 3, 1),
              image_pair=[a.transpose(0, 2, 3, 1), b.transpose(0, 2, 3, 1)], num_inference_steps=1, guidance_scale=3.0, latents=inp["x_T"])
    pipe = PromptDiffusionPipeline(e)
    lat = np.asarray(pipe(output_type="latent", **kw).images, np.float32)
    plain = pipe(output_type="np", **kw).images
    e.set_vae_tiling(False, tile_latent=8)                            # parameters on the engine, the switch on the pipeline
    pipe.enable_vae_tiling()
    assert e.vae_tiling[:3] == (True, False, 8)
    tiled = pipe(output_type="np", **kw).images
    want = np.clip(e.vae_decode(lat) / 2 + 0.5, 0, 1).transpose(0, 2, 3, 1)
    assert e.stat("vae_tiles") == 18
    pipe.disable_vae_tiling()
    again = pipe(output_type="np", **kw).images
    e.close()
    assert tiled.shape == plain.shape == (1, hw, hw, 3)
    assert np.array_equal(tiled, want)
    assert float(np.abs(tiled - plain).max()) > 1e-3                  # the tiled image is not the untiled one
    assert again.tobytes() == plain.tobytes()
