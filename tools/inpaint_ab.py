"""A/B of img2img / inpainting inside the engine's loop on the headline configuration (SD1.5, bs 8, 512x512, 50-step DDIM,
CFG 7.5, f16): the same engine and inputs sample plain, inpainting at strength 1.0 with a half-image mask, and img2img at
strength 0.6 (the last 30 of the 50 steps), alternating pass by pass so that clock and thermal drift hit every leg alike.
Prints one JSON line: images/s of each leg, launches per denoising step, and the per-step time of each leg against plain.

    python tools/inpaint_ab.py [--passes 3] [--batch 8] [--size 512] [--precision f16]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from prompt_diffusion_amd import engine as E  # noqa: E402
from prompt_diffusion_amd import weights as W  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3, help="timed passes per leg (each = one full sampling of the batch)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--strength", type=float, default=0.6, help="img2img leg")
    ap.add_argument("--precision", default="f16", choices=["f16", "bf16", "f16x2", "f32"])
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = W.SD15
    B, h, S = args.batch, args.size // 8, args.steps
    eng = E.Engine(cfg, device=0, precision=args.precision)
    eng.init_random_weights(1234)
    gen = torch.Generator(device=dev).manual_seed(2023)
    kw = dict(x_T=torch.randn((B, 4, h, h), generator=gen, device=dev),
              ctx_cond=torch.randn((B, cfg.context_len, cfg.context_dim), generator=gen, device=dev),
              ctx_uncond=torch.randn((B, cfg.context_len, cfg.context_dim), generator=gen, device=dev),
              pair=torch.rand((B, 6, 8 * h, 8 * h), generator=gen, device=dev) * 2 - 1,
              query=torch.rand((B, 3, 8 * h, 8 * h), generator=gen, device=dev) * 2 - 1,
              steps=S, cfg_scale=7.5, eta=0.0)
    z0 = torch.randn((B, 4, h, h), generator=gen, device=dev) * 0.8
    mask = torch.zeros((1, 1, h, h), device=dev)
    mask[..., h // 2:] = 1.0
    grid = [int(t) for t in (torch.arange(0, cfg.timesteps, cfg.timesteps // S) + 1).flip(0)]   # the 50-step grid, sampling order
    tail = grid[S - min(int(S * args.strength), S):]
    legs = {"plain": dict(),
            "inpaint_s1.0": dict(init_latents=z0, mask=mask, init_pure_noise=True),
            f"img2img_s{args.strength}": dict(init_latents=z0, timesteps=tail)}
    steps = {"plain": S, "inpaint_s1.0": S, f"img2img_s{args.strength}": len(tail)}

    times = {k: [] for k in legs}
    launches = {}
    for leg, extra in legs.items():   # warm-up; launches per step from a stepwise run (the fused loop launches the same)
        eng.ddim_sample(**kw, **extra)
        n = eng.sample_begin(**kw, **extra)
        c0 = eng.stat("launches")
        for i in range(n):
            eng.sample_step(i)
        launches[leg] = (eng.stat("launches") - c0) / n
        eng.sample_end()
    for _ in range(args.passes):
        for leg, extra in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = eng.ddim_sample(**kw, **extra)
            torch.cuda.synchronize()
            times[leg].append(time.perf_counter() - t0)
            assert torch.isfinite(out).all(), leg
    best = {k: min(v) for k, v in times.items()}
    per_step_ms = {k: 1e3 * best[k] / steps[k] for k in legs}
    print(json.dumps(dict(config=f"SD1.5 bs {B} {args.size}x{args.size} {S}-step DDIM {args.precision}",
                          images_per_s={k: round(B / v, 4) for k, v in best.items()},
                          steps=steps, launches_per_step=launches,
                          per_step_ms={k: round(v, 3) for k, v in per_step_ms.items()},
                          per_step_vs_plain_pct={k: round(100.0 * (v / per_step_ms["plain"] - 1.0), 3) for k, v in per_step_ms.items()},
                          pass_s={k: [round(t, 4) for t in v] for k, v in times.items()})))
    eng.close()


if __name__ == "__main__":
    main()
