"""First-stage KL-VAE encoder on the GPU (pd_vae_encode, Engine.vae_encode, the (L) facade's encode_first_stage) against the
reference Encoder's own outputs (tests/golden/vae_encoder.npz, make_golden_vae_encoder.py) and against torch on the CPU.

Moments bounds (max |diff| / max |ref|) are the decoder's: f32 1e-4, f16x2 1e-4, f16 4e-3, bf16 3e-2."""
import dataclasses
import os

import numpy as np
import pytest

from prompt_diffusion_amd import ddim as D
from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import weights as W

pytestmark = pytest.mark.gpu

TOL = {"f32": 1e-4, "f16x2": 1e-4, "f16": 4e-3, "bf16": 3e-2}
TINY_E = dataclasses.replace(W.TINY, vae_encoder=True)
SD15_E = dataclasses.replace(W.SD15, vae_encoder=True)


def relerr(a, b):
    return float(np.abs(np.asarray(a) - b).max() / (np.abs(b).max() + 1e-30))


def images_from_key(key, shape):   # tests/golden/make_golden_vae_encoder.py
    return np.random.Generator(np.random.Philox(key=[77, int(key)])).uniform(-1.0, 1.0, shape).astype(np.float32)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "vae_encoder.npz"))


def _encoder_engine(cfg, prec, full=False):
    e = E.Engine(cfg, precision=prec)
    for n, a in W.synth_vae_encoder_state_dict(cfg).items():
        e.load_tensor(n, a)
    if full:
        for n, a in W.synth_vae_state_dict(cfg).items():
            e.load_tensor(n, a)
        e.load_state_dict(W.synth_state_dict(cfg))
    assert e.vae_encoder_weights_missing() == 0
    return e


@pytest.fixture(scope="module")
def tiny_f32():
    e = _encoder_engine(TINY_E, "f32", full=True)
    yield e
    e.close()


@pytest.mark.parametrize("prec", ["f32", "f16x2", "f16", "bf16"])
@pytest.mark.parametrize("tag,cfg", [("tiny", TINY_E), ("sd15", SD15_E)])
def test_moments_match_reference(fx, tag, cfg, prec):
    e = _encoder_engine(cfg, prec)
    assert e.weights_missing() > 0 and e.vae_weights_missing() > 0   # the encoder needs neither the networks nor the decoder
    m = e.vae_encode(fx[tag + "_images"], mode="moments")
    assert m.shape == fx[tag + "_moments"].shape
    err = relerr(m, fx[tag + "_moments"])
    print(f"{tag} {prec}: moments relerr {err:.3e}")
    assert err < TOL[prec]
    e.close()


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_non_square_moments(fx, prec):
    e = _encoder_engine(TINY_E, prec)
    m = e.vae_encode(fx["nonsq_images"], mode="moments")
    assert m.shape == (1, 8, 8, 16)
    assert relerr(m, fx["nonsq_moments"]) < TOL[prec]
    e.close()


def test_sd15_512_f16_on_the_patch_kernels(fx, capfd):
    """The real dispatch: 128 channels at 512x512 and 256 at 256x256 run their 3x3 stride-1 convs on the LDS-patch kernels."""
    e = _encoder_engine(SD15_E, "f16")
    x = images_from_key(int(fx["sd15_512_key"]), (1, 3, 512, 512))
    capfd.readouterr()
    e.set_option("verbose", 2)
    m = e.vae_encode(x, mode="moments")
    e.set_option("verbose", 0)
    err = relerr(m, fx["sd15_512_moments"])
    print(f"sd15 512x512 f16: moments relerr {err:.3e}")
    assert err < TOL["f16"]
    lines = [l for l in capfd.readouterr().err.splitlines() if l.startswith("[pdengine] gemm")]
    for rows in (512 * 512, 256 * 256):
        big = [l for l in lines if f"M {rows} " in l and "taps 9 stride 1" in l and " K 72 " not in l]   # not conv_in (3 -> 8 channels)
        assert big and all("patch" in l for l in big), big
    down = [l for l in lines if "taps 9 stride 2" in l]
    assert len(down) == len(W.SD15.vae_ch_mult) - 1 and all("igemm" in l for l in down)
    e.close()


def test_mean_sample_moments_modes(fx):
    """MEAN / SAMPLE are the posterior of the engine's own MOMENTS to fp32 rounding, and the reference's within the f32 bound;
    MOMENTS returns logvar unclamped while SAMPLE clamps it to [-30, 20]."""
    cfg = TINY_E
    e = _encoder_engine(cfg, "f32")
    x, noise = fx["tiny_images"], fx["tiny_noise"]
    mom = e.vae_encode(x, mode="moments")
    mean = e.vae_encode(x, mode="mean")
    smp = e.vae_encode(x, mode="sample", noise=noise)
    sf = np.float32(cfg.scale_factor)
    mu, lv = mom[:, :4], np.clip(mom[:, 4:], -30.0, 20.0)
    assert relerr(mean, sf * mu) <= 1e-6
    assert relerr(smp, sf * (mu + np.exp(np.float32(0.5) * lv) * noise)) <= 1e-6
    assert relerr(mean, fx["tiny_mode"]) < TOL["f32"] and relerr(smp, fx["tiny_sample"]) < TOL["f32"]
    # push logvar out of the clamp range through quant_conv's bias: +-50 on the logvar rows
    name = "first_stage_model.quant_conv.bias"
    b = W.synth_vae_encoder_state_dict(cfg)[name].copy()
    b[4:6] += 50.0
    b[6:8] -= 50.0
    e.load_tensor(name, b)
    mom = e.vae_encode(x, mode="moments")
    assert mom[:, 4:6].min() > 20.0 and mom[:, 6:8].max() < -30.0       # unclamped
    smp = e.vae_encode(x, mode="sample", noise=noise)
    lv = np.clip(mom[:, 4:], -30.0, 20.0)
    assert relerr(smp, sf * (mom[:, :4] + np.exp(np.float32(0.5) * lv) * noise)) <= 1e-6
    e.close()


@pytest.mark.parametrize("prec,tol", [("f32", 1e-5), ("f16x2", 1e-4), ("f16", 4e-3), ("bf16", 3e-2)])
@pytest.mark.parametrize("B,Cc,H,Wd", [(2, 20, 13, 10), (1, 64, 34, 18), (3, 8, 7, 9)])
def test_op_vae_downsample_matches_torch(prec, tol, B, Cc, H, Wd):
    import torch
    import torch.nn.functional as F
    g = np.random.default_rng(B * 1000 + H)
    x = g.uniform(-1, 1, (B, Cc, H, Wd)).astype(np.float32)
    w = (g.standard_normal((Cc, Cc, 3, 3)) / np.sqrt(9 * Cc)).astype(np.float32)
    b = (0.1 * g.standard_normal(Cc)).astype(np.float32)
    ref = F.conv2d(F.pad(torch.from_numpy(x), (0, 1, 0, 1)), torch.from_numpy(w), torch.from_numpy(b), stride=2).numpy()
    sym = F.conv2d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), stride=2, padding=1).numpy()
    e = E.Engine(W.TINY, precision=prec)
    y = e.op_vae_downsample(x, w, b)
    assert y.shape == ref.shape == (B, Cc, H // 2, Wd // 2)
    assert relerr(y, ref) < tol
    if sym.shape == ref.shape:
        assert relerr(sym, ref) > 10 * tol   # the symmetric pad is a different function: this test tells them apart
    e.close()


def test_decoder_unaffected_by_the_encoder(fx):
    g = np.random.Generator(np.random.Philox(key=[5, 5]))
    z = g.standard_normal((2, 4, 8, 8), dtype=np.float32)
    outs, names = [], []
    for cfg in (W.TINY, TINY_E):
        e = E.Engine(cfg, precision="f32")
        for n, a in W.synth_vae_state_dict(cfg).items():
            e.load_tensor(n, a)
        if cfg.vae_encoder:
            for n, a in W.synth_vae_encoder_state_dict(cfg).items():
                e.load_tensor(n, a)
            e.vae_encode(fx["tiny_images"])
        outs.append(e.vae_decode(z))
        names.append(e.param_names())
        assert e.vae_weights_missing() == 0
        e.close()
    np.testing.assert_array_equal(outs[0], outs[1])
    assert names[1] == names[0] + [(n, tuple(s)) for n, s, _ in W.vae_encoder_spec(W.TINY)]


def test_batch_and_device_tensors(fx, tiny_f32):
    import torch
    x1 = fx["tiny_images"][:1]
    one = tiny_f32.vae_encode(x1, mode="moments")
    eight = tiny_f32.vae_encode(np.repeat(x1, 8, axis=0), mode="moments")
    for i in range(8):
        assert relerr(eight[i:i + 1], one) <= 1e-6
    x, noise = fx["tiny_images"], fx["tiny_noise"]
    for mode in ("mean", "sample", "moments"):
        host = tiny_f32.vae_encode(x, mode=mode, noise=noise if mode == "sample" else None)
        dev = tiny_f32.vae_encode(torch.from_numpy(x).cuda(), mode=mode,
                                  noise=torch.from_numpy(noise).cuda() if mode == "sample" else None)
        assert dev.is_cuda
        np.testing.assert_array_equal(dev.cpu().numpy(), host)


def _sample_kw(B=1, h=8, w=8):
    inp = W.synth_inputs(W.TINY, B, h, w)
    return dict(x_T=inp["x_T"], ctx_cond=inp["ctx_cond"], ctx_uncond=inp["ctx_uncond"], pair=inp["pair"], query=inp["query"],
                steps=4, cfg_scale=7.5)


def test_encode_decode_encode_then_sample(fx, tiny_f32):
    fresh = _encoder_engine(TINY_E, "f32", full=True)
    want = fresh.ddim_sample(**_sample_kw())
    fresh.close()
    x = fx["tiny_images"]
    m0 = tiny_f32.vae_encode(x, mode="moments")
    img = tiny_f32.vae_decode(tiny_f32.vae_encode(x, mode="mean"))
    assert img.shape == x.shape
    m1 = tiny_f32.vae_encode(x, mode="moments")
    np.testing.assert_array_equal(m0, m1)
    got = tiny_f32.ddim_sample(**_sample_kw())
    np.testing.assert_array_equal(got, want)


def test_refused_inputs(fx, tiny_f32):
    x = fx["tiny_images"]
    plain = E.Engine(W.TINY, precision="f32")
    with pytest.raises(E.PdError, match="without a VAE encoder"):
        plain.vae_encode(x)
    assert plain.vae_encoder_weights_missing() == 0
    plain.close()
    partial = E.Engine(TINY_E, precision="f32")
    with pytest.raises(E.PdError, match="'first_stage_model.encoder.conv_in.weight'"):
        partial.vae_encode(x)
    partial.close()
    e = tiny_f32
    e.sample_begin(**_sample_kw())
    with pytest.raises(E.PdError, match="end the sampling session first"):
        e.vae_encode(x)
    e.sample_end()
    with pytest.raises(E.PdError, match="multiples of 8"):
        e.vae_encode(np.zeros((1, 3, 60, 64), np.float32))
    with pytest.raises(E.PdError, match="multiple of 64"):
        e.vae_encode(np.zeros((1, 3, 64, 72), np.float32))
    out = np.empty((2, 4, 8, 8), np.float32)
    assert e.lib.pd_vae_encode(e._h, x.ctypes.data, 2, 64, 64, E.PD_MEM_HOST, 7, None, out.ctypes.data) != 0
    assert "unknown `what`" in e.lib.pd_last_error().decode()
    with pytest.raises(E.PdError, match="needs `noise`"):
        e.vae_encode(x, mode="sample")
    # still usable
    assert relerr(e.vae_encode(x, mode="moments"), fx["tiny_moments"]) < TOL["f32"]


def test_img2img_through_the_facade(fx, tiny_f32):
    """init = get_first_stage_encoding(encode_first_stage(x)) -> stochastic_encode -> decode (the SD img2img recipe) on the
    engine, against the same chain started from the reference's latents."""
    model = D.ControlLDM(tiny_f32)
    sampler = D.DDIMSampler(model)
    x, noise = fx["tiny_images"], fx["tiny_noise"]
    init = model.get_first_stage_encoding(model.encode_first_stage(x), noise=noise)
    assert relerr(init, fx["tiny_sample"]) < TOL["f32"]
    inp = W.synth_inputs(W.TINY, 2, 8, 8)
    cond = {"c_crossattn": [inp["ctx_cond"]], "example_pair": [inp["pair"]], "query": [inp["query"]]}
    unc = {"c_crossattn": [inp["ctx_uncond"]], "example_pair": [inp["pair"]], "query": [inp["query"]]}
    sampler.make_schedule(ddim_num_steps=10, ddim_eta=0.0, verbose=False)
    t_enc = 6
    q_noise = np.random.Generator(np.random.Philox(key=[9, 9])).standard_normal(init.shape, dtype=np.float32)

    def chain(z0):
        z = sampler.stochastic_encode(z0, np.full(2, t_enc, np.int64), noise=q_noise)
        return sampler.decode(z, cond, t_enc, unconditional_guidance_scale=7.5, unconditional_conditioning=unc)

    got, want = chain(init), chain(fx["tiny_sample"])
    err = relerr(got, want)
    print(f"img2img latents relerr {err:.3e} (init {relerr(init, fx['tiny_sample']):.3e})")
    assert err < 2e-4
    img = model.decode_first_stage(got)
    assert img.shape == x.shape and np.isfinite(img).all()
