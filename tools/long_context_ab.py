"""Long contexts measured on one box, alternating runs ("Long prompts"):

  block   the SD1.5 input_blocks.1.1. SpatialTransformer at the headline shape (forward batch 16, 64 x 64 tokens, f16) through
          op_spatial_transformer with option "profile" on: the sum of the HIP-event brackets around the block's contraction launches
          (fused front + self-attention + fused tail, or the per-layer path's GEMMs and attentions -- its LayerNorm / GroupNorm launches
          carry no bracket, so the per-layer figure is a lower bound), for st_fuse on / off at each context length.
  sample  a bench.py-shaped run (SD1.5, 512 x 512, 50-step DDIM, CFG 7.5, bs 8, f16, random weights) at each context length, st_fuse
          on / off, in images / s.

    python tools/long_context_ab.py [--lengths 77,231] [--rounds 3] [--skip-sample] [--skip-block]

The script also runs in a checkout of an older commit without per-call context lengths (there: --lengths 77), which is how the
"no regression at 77" comparison is made: one run per checkout, alternating."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PRE, BLK = "model.diffusion_model.", "input_blocks.1.1."


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", default="77,231")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-sample", action="store_true")
    ap.add_argument("--skip-block", action="store_true")
    args = ap.parse_args()
    from prompt_diffusion_amd import engine as E
    from prompt_diffusion_amd import weights as W
    lengths = [int(v) for v in args.lengths.split(",")]
    res = {"lib": E.LIB_PATH, "block_ms": {}, "sample_images_per_s": {}}
    cfg = W.SD15
    e = E.Engine(cfg, precision="f16")
    e.init_random_weights(1234)
    new_abi = hasattr(e.lib, "pd_op_spatial_transformer_ctx")

    if not args.skip_block:
        r = np.random.default_rng(0)
        x = r.standard_normal((16, 320, 64, 64), dtype=np.float32)
        ctxs = {L: r.standard_normal((16, L, 768), dtype=np.float32) for L in lengths}

        def block(L, fuse):
            e.set_option("st_fuse", fuse)
            e.op_spatial_transformer(PRE + BLK, x, ctxs[L])          # warm (weights repacked after the option change)
            e.set_option("profile", 1)
            e.op_spatial_transformer(PRE + BLK, x, ctxs[L])
            ms, n, _ = e.profile_read(-1)
            e.set_option("profile", 0)
            return ms, n
        for rnd in range(args.rounds):
            for L in lengths:
                if L != cfg.context_len and not new_abi:
                    continue
                for fuse in (1, 0):
                    ms, n = block(L, fuse)
                    res["block_ms"].setdefault(f"L{L}_fuse{fuse}", []).append(round(ms, 4))
                    res.setdefault("block_launches", {})[f"L{L}_fuse{fuse}"] = n
        e.set_option("st_fuse", 1)

    if not args.skip_sample:
        import torch
        dev = torch.device("cuda:0")
        gen = torch.Generator(device=dev).manual_seed(2023)
        B, S, h, w = 8, 50, 64, 64
        base = dict(x_T=torch.randn((B, 4, h, w), generator=gen, device=dev),
                    pair=torch.rand((B, 6, 8 * h, 8 * w), generator=gen, device=dev) * 2 - 1,
                    query=torch.rand((B, 3, 8 * h, 8 * w), generator=gen, device=dev) * 2 - 1, steps=S, cfg_scale=7.5, eta=0.0)
        ctx = {L: (torch.randn((B, L, 768), generator=gen, device=dev), torch.randn((B, L, 768), generator=gen, device=dev)) for L in lengths}

        def sample(L, fuse):
            e.set_option("st_fuse", fuse)
            kw = dict(base, ctx_cond=ctx[L][0], ctx_uncond=ctx[L][1])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = e.ddim_sample(**kw)
            torch.cuda.synchronize()
            assert torch.isfinite(out).all()
            return B / (time.perf_counter() - t0)
        for L in lengths:                       # warm-up: workspace growth, weight repacking
            if L == cfg.context_len or new_abi:
                sample(L, 1), sample(L, 0)
        for rnd in range(args.rounds):
            for L in lengths:
                if L != cfg.context_len and not new_abi:
                    continue
                for fuse in (1, 0):
                    res["sample_images_per_s"].setdefault(f"L{L}_fuse{fuse}", []).append(round(sample(L, fuse), 4))
    e.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
