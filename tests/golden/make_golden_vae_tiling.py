#!/usr/bin/env python3
"""Generate tests/golden/vae_tiling.npz: tiled VAE decode / encode, from the REFERENCE's own layers.

The reference's unmodified Decoder / Encoder (ldm/modules/diffusionmodules/model.py) with post_quant_conv / quant_conv
(ldm/models/autoencoder.py:33-34) run PER TILE on the CPU with the synthetic weights of prompt-diffusion_amd/weights.py (W.TINY), and
tests/vae_tiling_ref.py -- diffusers' sequential tiled_decode / tiled_encode -- blends, crops and concatenates the tiles.  Only data is
stored:

  dec_z [1, 4, 32, 20]          the latent (the test decodes it with tile_latent 16, overlap 0.25: a 3 x 2 grid, tile sides 16, 16, 8 by 16, 8)
  dec_tiled [1, 3, 256, 160]    decode_first_stage with tiling: tiles of 1 / scale_factor * z
  dec_untiled (float16)         the same latent decoded in one piece: what the tiled result must NOT be
  enc_key                       the image is images_from_key(enc_key, [1, 3, 256, 160]) (tiles of 128, 128, 64 by 128, 64 pixels)
  enc_tiled [1, 8, 32, 20]      the assembled moments
  enc_untiled                   the moments of the whole image
  dec_differs / enc_differs     names of the precisions whose bound (1e-4 / 1e-4 / 4e-3 / 3e-2) the tiled and the untiled result are
                                apart by more than 10 times: there the GPU test also asserts "not the untiled result"

Usage: python tests/golden/make_golden_vae_tiling.py --reference DIR
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import install_stubs, t2n  # noqa: E402
from make_golden_vae_encoder import build as build_encoder, images_from_key  # noqa: E402
import vae_tiling_ref as R  # noqa: E402

TOL = {"f32": 1e-4, "f16x2": 1e-4, "f16": 4e-3, "bf16": 3e-2}
T, F = 16, 0.25


def build_decoder(cfg, W):
    from ldm.modules.diffusionmodules.model import Decoder
    dec = Decoder(ch=cfg.vae_ch, out_ch=cfg.vae_out_ch, ch_mult=cfg.vae_ch_mult, num_res_blocks=cfg.vae_num_res_blocks,
                  attn_resolutions=[], dropout=0.0, in_channels=3, resolution=256, z_channels=cfg.in_channels)
    pq = torch.nn.Conv2d(cfg.in_channels, cfg.in_channels, 1)
    spec = {n[len(W.VAE_PREFIX):]: (s_, k) for n, s_, k in W.vae_spec(cfg)}
    dec.load_state_dict({k: torch.from_numpy(W.synth_tensor(W.VAE_PREFIX + "decoder." + k, v.shape, spec["decoder." + k][1]))
                         for k, v in dec.state_dict().items()})
    pq.load_state_dict({k: torch.from_numpy(W.synth_tensor(W.VAE_PREFIX + "post_quant_conv." + k, v.shape, spec["post_quant_conv." + k][1]))
                        for k, v in pq.state_dict().items()})
    dec.eval()
    return dec, pq


def relerr(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, metavar="DIR", help="checkout of the reference project")
    args = ap.parse_args()
    install_stubs()
    sys.path.insert(0, os.path.abspath(args.reference))
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from prompt_diffusion_amd import weights as W
    torch.set_num_threads(8)
    cfg = W.TINY
    res = {}

    dec, pq = build_decoder(cfg, W)
    z = np.random.Generator(np.random.Philox(key=[91, 1])).standard_normal((1, cfg.in_channels, 32, 20), dtype=np.float32)
    zs = t2n(1.0 / cfg.scale_factor * torch.from_numpy(z))   # ddpm.py:827: the scaling comes before the (tiled) decode
    with torch.no_grad():
        fn = lambda t: t2n(dec(pq(torch.from_numpy(np.ascontiguousarray(t)))))
        tiled = R.tiled_decode(zs, T, F, fn)
        untiled = fn(zs)
    assert tiled.shape == untiled.shape == (1, 3, 256, 160)
    sep = relerr(tiled, untiled)
    res.update(dec_z=z, dec_tiled=tiled, dec_untiled=untiled.astype(np.float16),
               dec_differs=np.array([p for p, t in TOL.items() if sep > 10 * t]))
    print(f"[golden] vae_tiling decode: tiled vs untiled {sep:.3e}; 'differs' asserted for {list(res['dec_differs'])}")

    enc, qc, _ = build_encoder(cfg, W)
    key = 7
    x = images_from_key(key, (1, cfg.vae_out_ch, 256, 160))
    with torch.no_grad():
        fn = lambda t: t2n(qc(enc(torch.from_numpy(np.ascontiguousarray(t)))))
        tiled = R.tiled_encode(x, T, F, fn)
        untiled = fn(x)
    assert tiled.shape == untiled.shape == (1, 2 * cfg.in_channels, 32, 20)
    sep = relerr(tiled, untiled)
    res.update(enc_key=np.array(key, np.int64), enc_tiled=tiled, enc_untiled=untiled,
               enc_differs=np.array([p for p, t in TOL.items() if sep > 10 * t]))
    print(f"[golden] vae_tiling encode: tiled vs untiled {sep:.3e}; 'differs' asserted for {list(res['enc_differs'])}")
    for p in ("f32", "f16x2", "f16"):   # (bf16 keeps the parity assertion alone where the separation is not there)
        assert p in res["dec_differs"] and p in res["enc_differs"], p
    np.savez_compressed(os.path.join(HERE, "vae_tiling.npz"), **res)


if __name__ == "__main__":
    main()
