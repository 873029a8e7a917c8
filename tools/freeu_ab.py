"""A/B of FreeU's cost on the headline configuration (SD1.5, bs 8, 512x512, 50-step DDIM, CFG 7.5, f16): the same engine and
inputs sample with FreeU off and on (0.9, 0.2, 1.5, 1.6), alternating pass by pass so that clock and thermal drift hit both
legs alike.  Prints one JSON line: images/s of each leg, the relative cost, and launches per denoising step.

    python tools/freeu_ab.py [--passes 3] [--batch 8] [--size 512] [--precision f16]
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
    ap.add_argument("--precision", default="f16", choices=["f16", "bf16", "f16x2", "f32"])
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = W.SD15
    B, h = args.batch, args.size // 8
    eng = E.Engine(cfg, device=0, precision=args.precision)
    eng.init_random_weights(1234)
    gen = torch.Generator(device=dev).manual_seed(2023)
    kw = dict(x_T=torch.randn((B, 4, h, h), generator=gen, device=dev),
              ctx_cond=torch.randn((B, cfg.context_len, cfg.context_dim), generator=gen, device=dev),
              ctx_uncond=torch.randn((B, cfg.context_len, cfg.context_dim), generator=gen, device=dev),
              pair=torch.rand((B, 6, 8 * h, 8 * h), generator=gen, device=dev) * 2 - 1,
              query=torch.rand((B, 3, 8 * h, 8 * h), generator=gen, device=dev) * 2 - 1,
              steps=args.steps, cfg_scale=7.5, eta=0.0)
    legs = {"off": None, "on": (0.9, 0.2, 1.5, 1.6)}

    def use(leg):
        if legs[leg] is None:
            eng.disable_freeu()
        else:
            eng.set_freeu(*legs[leg])

    times = {k: [] for k in legs}
    launches = {}
    outs = {}
    for leg in legs:   # warm-up, launch count
        use(leg)
        n0 = eng.stat("launches")
        outs[leg] = eng.ddim_sample(**kw)
        torch.cuda.synchronize()
        launches[leg] = (eng.stat("launches") - n0) / args.steps
    for _ in range(args.passes):
        for leg in legs:
            use(leg)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = eng.ddim_sample(**kw)
            torch.cuda.synchronize()
            times[leg].append(time.perf_counter() - t0)
            assert torch.isfinite(out).all(), leg
    rate = {k: B / min(v) for k, v in times.items()}
    diff = float((outs["on"] - outs["off"]).abs().max() / outs["off"].abs().max())
    print(json.dumps(dict(config=f"SD1.5 bs {B} {args.size}x{args.size} {args.steps}-step DDIM {args.precision}",
                          images_per_s_off=round(rate["off"], 4), images_per_s_on=round(rate["on"], 4),
                          cost_pct=round(100.0 * (rate["off"] / rate["on"] - 1.0), 3),
                          pass_s_off=[round(t, 4) for t in times["off"]], pass_s_on=[round(t, 4) for t in times["on"]],
                          launches_per_step_off=launches["off"], launches_per_step_on=launches["on"],
                          latent_relchange_on_vs_off=round(diff, 4))))
    eng.close()


if __name__ == "__main__":
    main()
