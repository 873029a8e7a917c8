"""SD3's VAE on the GPU (pd_sd3_vae_*, SD3Engine.vae_encode / vae_decode, the pipeline's image ends) against the reference
Encoder's / Decoder's own outputs (tests/golden/sd3_vae.npz, make_golden_sd3_vae.py).

Bounds (max |diff| / max |ref|) are the SD1.5 first stage's: f32 1e-4, f16x2 1e-4, f16 4e-3, bf16 3e-2.  The 2-byte modes run
the mid-block attention on the flash kernel (vae_flash 1) and on the materialised path (0); the fp32-storage modes materialise."""
import os

import numpy as np
import pytest

from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import sd3
from prompt_diffusion_amd import weights as W
from prompt_diffusion_amd.pipeline_sd3 import StableDiffusion3PromptDiffusionPipeline as Pipe
from tests import sd3_vae_ref as R

pytestmark = pytest.mark.gpu

TOL = {"f32": 1e-4, "f16x2": 1e-4, "f16": 4e-3, "bf16": 3e-2}
# the smallest SD3 networks that take the VAE's 16 latent channels
NET = sd3.SD3Config(in_channels=16, out_channels=16, heads=2, head_dim=64, layers=2, cn_layers=1, joint_dim=96, pooled_dim=40,
                    pos_embed_max_size=12)
VAES = {"tiny": sd3.SD3_TINY_VAE, "full": sd3.SD3_MEDIUM_VAE}
MODES = [("f32", 0), ("f16x2", 0), ("f16", 0), ("f16", 1), ("bf16", 0), ("bf16", 1)]


def relerr(a, b):
    return float(np.abs(np.asarray(a) - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "sd3_vae.npz"))


def vae_engine(fx, which, prec, encoder=True, net=False):
    e = sd3.SD3Engine(NET, precision=prec)
    e.configure_vae(VAES[which], encoder=encoder)
    sd = sd3.synth_sd3_vae_state_dict(VAES[which], int(fx["seed"]))
    if net:
        sd.update(sd3.synth_sd3_state_dict(NET))
    e.load_state_dict(sd, strict=net)
    assert e.vae_weights_missing() == 0
    return e


@pytest.fixture(scope="module")
def tiny_f32(fx):
    e = vae_engine(fx, "tiny", "f32", net=True)
    yield e
    e.close()


def images(fx, tag):
    if tag + "_images" in fx:
        return fx[tag + "_images"]
    B, H, Wd = (int(v) for v in fx[tag + "_shape"])
    return R.images_from_key(int(fx[tag + "_key"]), (B, 3, H, Wd))


@pytest.mark.parametrize("prec,flash", MODES)
@pytest.mark.parametrize("which", ["tiny", "full"])
def test_moments_and_decoded_match_reference(fx, which, prec, flash):
    """All four cases: the square one and the 12 x 20 latents (N = 240: no multiple of a query block, a key tile or 64)."""
    e = vae_engine(fx, which, prec)
    assert e.weights_missing() > 0                       # the VAE needs neither network
    e.base.set_option("vae_flash", flash)
    for tag in (which, which + "_nonsq"):
        n0 = e.base.stat("vae_flash_launches")
        m = e.vae_encode(images(fx, tag), mode="moments")
        d = e.vae_decode(fx[tag + "_z"], raw=True)
        assert e.base.stat("vae_flash_launches") - n0 == 2 * flash
        assert m.shape == fx[tag + "_moments"].shape and d.shape == fx[tag + "_decoded"].shape
        em, ed = relerr(m, fx[tag + "_moments"]), relerr(d, fx[tag + "_decoded"])
        print(f"{tag} {prec} flash {flash}: moments {em:.3e} decoded {ed:.3e} (bound {TOL[prec]:g})")
        assert em < TOL[prec] and ed < TOL[prec]
    e.close()


def test_which_path_the_default_takes(fx):
    """Option vae_flash at its default -1: SD3's VAE materialises where that measures faster (the score buffers of these sizes are
    far below 2 GiB) and takes the flash kernel where the materialised GEMMs cannot run (h * w no multiple of 8); fp32 storage
    materialises whatever the option says."""
    e = vae_engine(fx, "tiny", "bf16")
    e.vae_decode(fx["tiny_z"], raw=True)
    assert e.base.stat("vae_flash_launches") == 0
    z = R.latents_from_key(9, (1, 16, 3, 5))                  # N = 15
    d = e.vae_decode(z)
    assert e.base.stat("vae_flash_launches") == 1 and d.shape == (1, 3, 24, 40) and np.isfinite(d).all()
    e.base.set_option("vae_flash", 1)
    assert np.array_equal(e.vae_decode(z), d)
    e.base.set_option("vae_flash", 0)
    with pytest.raises(E.PdError, match="multiple of 8"):
        e.vae_decode(z)
    e.close()
    e = vae_engine(fx, "tiny", "f32")
    e.base.set_option("vae_flash", 1)
    e.vae_decode(fx["tiny_z"], raw=True)
    assert e.base.stat("vae_flash_launches") == 0
    e.close()


def test_sample_and_mode_with_shift_and_scaling(fx, tiny_f32):
    e = tiny_f32
    s = e.vae_encode(fx["tiny_images"], mode="sample", noise=fx["tiny_noise"])
    assert relerr(s, fx["tiny_sample"]) < TOL["f32"]
    assert relerr(e.vae_encode(fx["tiny_images"], mode="mean"), fx["tiny_mode"]) < TOL["f32"]


def test_raw_against_scaled(fx, tiny_f32):
    e, c = tiny_f32, sd3.SD3_TINY_VAE
    x = fx["tiny_images"]
    raw = e.vae_encode(x, mode="sample", noise=fx["tiny_noise"], raw=True)
    scaled = e.vae_encode(x, mode="sample", noise=fx["tiny_noise"])
    np.testing.assert_allclose(scaled, (raw - np.float32(c.shift_factor)) * np.float32(c.scaling_factor), rtol=2e-6, atol=1e-6)
    # moments know neither
    assert np.array_equal(e.vae_encode(x, mode="moments"), e.vae_encode(x, mode="moments", raw=True))
    # decode: latents / scaling + shift inside the layout kernel
    z = fx["tiny_z"]
    lat = ((z - np.float32(c.shift_factor)) * np.float32(c.scaling_factor)).astype(np.float32)
    assert relerr(e.vae_decode(lat), e.vae_decode(z, raw=True)) < 1e-5
    assert relerr(e.vae_decode(lat), fx["tiny_decoded"]) < TOL["f32"]


def test_seeded_sampling_is_reproducible(fx, tiny_f32):
    e = tiny_f32
    x = fx["tiny_images"]
    e.base.set_rng(1234)
    a = e.vae_encode(x, mode="sample")
    e.base.set_rng(1234)
    b = e.vae_encode(x, mode="sample")
    e.base.set_rng(1235)
    c = e.vae_encode(x, mode="sample")
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    # ... and it is the posterior's: (a - mode) / (scaling std) is the engine's own draw
    mom = e.vae_encode(x, mode="moments")
    std = np.exp(0.5 * np.clip(mom[:, 16:], -30.0, 20.0))
    e.base.set_rng(1234)
    z = e.base.randn((2, 16, 8, 8), "vae")
    want = (mom[:, :16] + std * z - np.float32(sd3.SD3_TINY_VAE.shift_factor)) * np.float32(sd3.SD3_TINY_VAE.scaling_factor)
    assert relerr(a, want) < 1e-5


def test_device_round_trip_equals_host_path(fx, tiny_f32):
    import torch
    e = tiny_f32
    x = fx["tiny_images"]
    lat_h = e.vae_encode(x, mode="mean")
    img_h = e.vae_decode(lat_h)
    xd = torch.from_numpy(x).cuda()
    lat_d = e.vae_encode(xd, mode="mean")
    img_d = e.vae_decode(lat_d)
    assert lat_d.is_cuda and img_d.is_cuda and tuple(img_d.shape) == (2, 3, 64, 64)
    assert np.array_equal(lat_d.cpu().numpy(), lat_h) and np.array_equal(img_d.cpu().numpy(), img_h)


def test_encode_support_pair_on_the_engine(fx, tiny_f32):
    e = tiny_f32
    g = np.random.default_rng(5)
    cond, gt = (g.uniform(-1, 1, (1, 3, 64, 64)).astype(np.float32) for _ in range(2))
    e.base.set_rng(77)
    got = e.encode_support_pair(cond, gt)
    e.base.set_rng(77)
    want = e.vae_encode(e.down_proj(cond, gt), mode="sample", raw=True)
    assert got.shape == (1, 16, 8, 8) and np.array_equal(got, want)


def test_error_paths(fx, tiny_f32):
    e = tiny_f32
    with pytest.raises(ValueError):
        e.vae_encode(np.zeros((1, 3, 60, 64), np.float32), mode="mean")          # not a multiple of 8
    with pytest.raises(ValueError):
        e.vae_encode(fx["tiny_images"], mode="nope")
    with pytest.raises(ValueError):
        e.vae_decode(np.zeros((1, 4, 8, 8), np.float32))
    with pytest.raises(E.PdError, match="multiple of 8"):
        e.vae_decode(np.zeros((1, 16, 3, 3), np.float32))                         # f32 materialises: h * w = 9
    with pytest.raises(E.PdError, match="already configured"):
        e.configure_vae(sd3.SD3_TINY_VAE)
    lib, h = e.base.lib, e.base._h
    out = np.zeros((1, 16, 8, 8), np.float32)
    x = np.zeros((1, 3, 64, 64), np.float32)
    assert lib.pd_sd3_vae_encode(h, x.ctypes.data, 1, 64, 64, E.PD_MEM_HOST, 7, None, 0, out.ctypes.data) != 0     # bad `what`
    assert lib.pd_sd3_vae_encode(h, None, 1, 64, 64, E.PD_MEM_HOST, 0, None, 0, out.ctypes.data) != 0
    # weights missing
    e2 = sd3.SD3Engine(NET, precision="f32")
    e2.configure_vae(sd3.SD3_TINY_VAE, encoder=False)
    assert e2.vae_weights_missing() == len(sd3.sd3_vae_spec(sd3.SD3_TINY_VAE, encoder=False))
    with pytest.raises(E.PdError, match="not loaded"):
        e2.vae_decode(fx["tiny_z"])
    with pytest.raises(E.PdError, match="no SD3 VAE encoder"):
        e2.vae_encode(fx["tiny_images"])
    e2.load_state_dict(sd3.synth_sd3_vae_state_dict(sd3.SD3_TINY_VAE, int(fx["seed"])), strict=False)   # the encoder's tensors are skipped
    assert e2.vae_weights_missing() == 0
    e2.close()


def test_engine_without_vae_is_unchanged(fx):
    e = sd3.SD3Engine(NET, precision="f32")
    names = [n for n, _ in e.base.param_names()]
    assert not any(n.startswith("vae.") for n in names)
    with pytest.raises(E.PdError, match="no SD3 VAE"):
        e.vae_decode(fx["tiny_z"])
    e.load_state_dict(sd3.synth_sd3_vae_state_dict(sd3.SD3_TINY_VAE), strict=False)     # skipped, like unconfigured text encoders
    n_before = len(names)
    e.configure_vae(sd3.SD3_TINY_VAE)
    after = [n for n, _ in e.base.param_names()]
    assert after[:n_before] == names and sorted(after[n_before:]) == sorted(n for n, _, _ in sd3.sd3_vae_spec(sd3.SD3_TINY_VAE))
    assert e.weights_missing() >= e.vae_weights_missing() == len(after) - n_before
    e.close()


def test_sd15_engine_is_unchanged(golden_dir):
    """A default SD1.5 engine: the same registry, vae_flash at its default 0 (no flash launch), and its decode of vae.npz's tiny case
    inside the fixture bound and bit-identical between two engines; with the option forced on, the flash kernel takes the same call."""
    g = np.load(os.path.join(golden_dir, "vae.npz"))
    z, ref = g["tiny_z"], g["tiny_x"]
    want_names = [n for n, _, _ in W.param_spec(W.TINY) + W.vae_spec(W.TINY) + W.text_spec(W.TINY)]   # tests/test_network_gpu.py's order
    outs = []
    for _ in range(2):
        e = E.Engine(W.TINY, precision="f16")
        names = [n for n, _ in e.param_names()]
        assert names == want_names
        for n, a in W.synth_vae_state_dict(W.TINY).items():
            e.load_tensor(n, a)
        outs.append(e.vae_decode(z))
        assert e.stat("vae_flash_launches") == 0
        assert relerr(outs[-1], ref) < TOL["f16"]
        e.close()
    assert np.array_equal(outs[0], outs[1])
    e = E.Engine(W.TINY, precision="f16")
    for n, a in W.synth_vae_state_dict(W.TINY).items():
        e.load_tensor(n, a)
    e.set_option("vae_flash", 1)
    fl = e.vae_decode(z)
    assert e.stat("vae_flash_launches") == 1 and relerr(fl, ref) < TOL["f16"]
    e.close()


def test_pipeline_end_to_end_equals_injected_engine_methods(fx, tiny_f32):
    """Image control_image, an image pair, output_type "np": the engine's VAE by default equals the same call with the engine's own
    methods injected as callables (which take the pipeline's older route)."""
    e = tiny_f32
    g = np.random.default_rng(9)
    f = lambda *s: g.standard_normal(s).astype(np.float32)
    img = g.uniform(0, 1, (1, 64, 64, 3)).astype(np.float32)                      # NHWC in [0, 1], like a PIL image as an array
    pair = [g.uniform(0, 1, (1, 3, 64, 64)).astype(np.float32) for _ in range(2)]
    kw = dict(prompt_embeds=f(1, 6, NET.joint_dim), pooled_prompt_embeds=f(1, NET.pooled_dim), negative_prompt_embeds=f(1, 6, NET.joint_dim),
              negative_pooled_prompt_embeds=f(1, NET.pooled_dim), control_image=img, control_image_pair=pair, latents=f(1, 16, 8, 8),
              num_inference_steps=2, guidance_scale=4.0, output_type="np")
    e.base.set_rng(5)
    a = Pipe(e)(**kw)["images"]
    assert a.shape == (1, 64, 64, 3) and np.isfinite(a).all() and a.min() >= 0.0 and a.max() <= 1.0 and a.std() > 1e-3
    e.base.set_rng(5)
    injected = Pipe(e, vae_encode=lambda x: e.vae_encode(x, mode="sample", raw=True), vae_decode=lambda z: e.vae_decode(z, raw=True),
                    down_proj=lambda p: e.down_proj(p[:, :3], p[:, 3:]))
    b = injected(**kw)["images"]
    assert np.array_equal(a, b)
    pil = Pipe(e)(**dict(kw, output_type="pil"))["images"]
    assert pil[0].size == (64, 64)
