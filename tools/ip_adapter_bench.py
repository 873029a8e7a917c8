"""What IP-Adapter costs on the headline configuration (SD1.5, bs 8, 512x512, 50-step DDIM, CFG 7.5, f16, random weights, 4 image tokens),
and the image term's kernel alone at the four UNet levels.

One engine, one process, the legs alternating pass by pass so that clock and thermal drift hit them alike; medians, with every pass listed:
    off          no image set: the engine launches what an engine without an adapter launches
    off_nofuse   the same with option st_fuse 0.  The option is global: it also unfuses the ControlNet's 320-channel blocks, which an active
                 adapter leaves fused, so this leg is an upper bound of what the adapter's bypass of the UNet's fused tails costs
    on           image set, scale 1
    zero         image set, scale 0 (must sit inside the run-to-run spread of `off`)
    on_other     scale 1 in the 11 blocks that have no fused tail (640 / 1280 channels), 0 in the others: the term's launches alone, in place
    on_320       scale 1 in the UNet's five 320-channel blocks, 0 in the others: their bypassed fused tails plus their ten launches per step
The split of `on` is attributed in "split_pct_of_off": the kernel = on_other + the ten 64 x 64 launches per step at their time alone
(kernel_alone); the bypassed UNet tails = on - off - the kernel.  Also pd_ip_adapter_set_image alone (projection, LayerNorm, 32 K / V
GEMMs, one synchronisation).  The kernel alone is timed by pd_bench_ip_attention next to a device-to-device copy of the 3 B N C elements it moves, in the same process.  Prints one JSON object.

    python tools/ip_adapter_bench.py [--passes 3] [--batch 8] [--size 512] [--precision f16] [--out profiles/ip_adapter_bench.json]
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from prompt_diffusion_amd import engine as E  # noqa: E402
from prompt_diffusion_amd import ip_adapter as IP  # noqa: E402
from prompt_diffusion_amd import weights as W  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3, help="timed passes per leg (each = one full sampling of the batch)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--tokens", type=int, default=4)
    ap.add_argument("--precision", default="f16", choices=["f16", "bf16", "f16x2", "f32"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = dataclasses.replace(W.SD15, ip_adapter=(args.tokens, 1024))
    B, h = args.batch, args.size // 8
    eng = E.Engine(cfg, device=0, precision=args.precision)
    eng.init_random_weights(1234)
    assert eng.ip_adapter_weights_missing() == 0
    gen = torch.Generator(device=dev).manual_seed(2023)
    kw = dict(x_T=torch.randn((B, 4, h, h), generator=gen, device=dev),
              ctx_cond=torch.randn((B, cfg.context_len, cfg.context_dim), generator=gen, device=dev),
              ctx_uncond=torch.randn((B, cfg.context_len, cfg.context_dim), generator=gen, device=dev),
              pair=torch.rand((B, 6, 8 * h, 8 * h), generator=gen, device=dev) * 2 - 1,
              query=torch.rand((B, 3, 8 * h, 8 * h), generator=gen, device=dev) * 2 - 1,
              steps=args.steps, cfg_scale=7.5, eta=0.0)
    emb = torch.randn((1, 1024), generator=gen, device=dev)

    tail = [1.0 if c == 320 else 0.0 for c in IP.block_widths(cfg)]      # the blocks whose fused tail a term bypasses
    scales = {"on": 1.0, "zero": 0.0, "on_320": tail, "on_other": [1.0 - t for t in tail]}

    def use(leg):
        eng.set_option("st_fuse", 0 if leg == "off_nofuse" else 1)
        if leg in ("off", "off_nofuse"):
            eng.ip_adapter_clear_image()
        else:
            eng.ip_adapter_set_scale(scales[leg])
            eng.ip_adapter_set_image(emb)

    legs = ("off", "off_nofuse", "on", "zero", "on_other", "on_320")
    times = {k: [] for k in legs}
    launches, ip_launches, outs = {}, {}, {}
    for leg in legs:   # warm-up, launch counts
        use(leg)
        n0, i0 = eng.stat("launches"), eng.stat("ip_launches")
        outs[leg] = eng.ddim_sample(**kw)
        torch.cuda.synchronize()
        launches[leg] = (eng.stat("launches") - n0) / args.steps
        ip_launches[leg] = (eng.stat("ip_launches") - i0) / args.steps
    for _ in range(args.passes):
        for leg in legs:
            use(leg)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = eng.ddim_sample(**kw)
            torch.cuda.synchronize()
            times[leg].append(time.perf_counter() - t0)
            assert torch.isfinite(out).all(), leg
    use("off")
    set_ms = []
    for _ in range(10):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.ip_adapter_set_image(emb)      # (synchronises before it returns)
        set_ms.append(1e3 * (time.perf_counter() - t0))
    eng.ip_adapter_clear_image()
    med = {k: statistics.median(v) for k, v in times.items()}
    rate = {k: B / med[k] for k in legs}
    spread_off = (max(times["off"]) - min(times["off"])) / med["off"]
    # the kernel alone at the four levels of this batch under guidance: one launch covers one guidance half (B samples)
    levels = []
    for ds, C in ((1, 320), (2, 640), (4, 1280), (8, 1280)):
        N = (h // ds) ** 2
        k_ms, c_ms = eng.bench_ip_attention(B, N, C, args.tokens, iters=50)
        moved = 3 * B * N * C * (4 if args.precision in ("f32", "f16x2") else 2)
        levels.append(dict(level=f"{h // ds}x{h // ds}", B=B, N=N, C=C, kernel_us=round(1e3 * k_ms, 2), copy_us=round(1e3 * c_ms, 2),
                           kernel_over_copy=round(k_ms / c_ms, 3), kernel_GBps=round(moved / (k_ms * 1e-3) / 1e9, 1)))
    # the split of `on`: the term's launches against the bypassed fused tails of the UNet's 320-channel blocks
    k64_s = 2 * sum(tail) * levels[0]["kernel_us"] * 1e-6 * args.steps          # their launches per pass, at the time of the kernel alone
    kernel_s = (med["on_other"] - med["off"]) + k64_s
    split = dict(kernel_other_blocks_measured=round(100 * (med["on_other"] - med["off"]) / med["off"], 3),
                 kernel_320_blocks_from_kernel_alone=round(100 * k64_s / med["off"], 3),
                 kernel=round(100 * kernel_s / med["off"], 3),
                 bypassed_unet_tails=round(100 * (med["on"] - med["off"] - kernel_s) / med["off"], 3),
                 on_320_plus_on_other_minus_on=round(100 * (med["on_320"] + med["on_other"] - med["off"] - med["on"]) / med["off"], 3))
    res = dict(config=f"SD1.5 bs {B} {args.size}x{args.size} {args.steps}-step DDIM {args.precision}, T = {args.tokens}, random weights",
               images_per_s={k: round(rate[k], 4) for k in legs},
               pass_s={k: [round(t, 4) for t in v] for k, v in times.items()},
               off_spread_pct=round(100 * spread_off, 3),
               cost_pct_vs_off={k: round(100.0 * (med[k] / med["off"] - 1.0), 3) for k in legs if k != "off"},
               split_pct_of_off=split, launches_per_step=launches, ip_launches_per_step=ip_launches,
               set_image_ms=dict(median=round(statistics.median(set_ms), 3), all=[round(t, 3) for t in set_ms]),
               zero_equals_off=bool(torch.equal(outs["zero"], outs["off"])),
               latent_relchange_on_vs_off=round(float((outs["on"] - outs["off"]).abs().max() / outs["off"].abs().max()), 4),
               kernel_alone=levels)
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    eng.close()


if __name__ == "__main__":
    main()
