"""What perturbed-attention guidance (pd_set_pag) costs on the headline configuration (SD1.5, bs 8, 512x512, 50-step DDIM, CFG 7.5, f16,
random weights), and the identity kernel alone at the four UNet levels.

One engine, one process, the legs alternating pass by pass so that clock and thermal drift hit them alike; medians, with every pass listed:
    off        no PAG: the engine launches what an engine that never heard of it launches
    zero       PAG set at scale 0 (must sit inside the run-to-run spread of `off`)
    mid        "mid", scale 3, the branch forked at the middle block (option pag_fork 1)
    mid_plain  the same with pag_fork 0: the perturbed branch a full third of the UNet's batch from conv_in on
    wide       ["down.block_2", "mid", "up.block_1"], fork on
Next to the measured cost, the share of the UNet's contraction FLOPs that the forked part of `mid` and `wide` adds, computed from
shapes (resblock convs and the transformer blocks' linear layers and attention products behind the fork, per sample, over the UNet +
ControlNet evaluation of the 2 B samples).  The kernel alone is timed by pd_bench_pag_identity next to a device-to-device copy of the
bytes it moves, in the same process.  Prints one JSON object.

    python tools/pag_bench.py [--passes 3] [--batch 8] [--size 512] [--precision f16] [--out profiles/pag_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from prompt_diffusion_amd import engine as E  # noqa: E402
from prompt_diffusion_amd import weights as W  # noqa: E402
from prompt_diffusion_amd.pag import parse_pag_layers  # noqa: E402


def unet_flops(cfg, h, blocks):
    """(contraction FLOPs of one sample through the UNet, of which behind the first block of the perturbed set `blocks` in evaluation
    order: the encoder's blocks, the middle block -- the last index --, the decoder's)"""
    L, D = cfg.context_len, cfg.context_dim

    def res(cin, cout, n):
        return 2 * n * 9 * cin * cout + 2 * n * 9 * cout * cout + (2 * n * cin * cout if cin != cout else 0)

    def st(c, n):      # proj_in, q k v, to_out, q2, to_out2, GEGLU in / out, proj_out; the two attention products; the context k / v
        return 2 * n * c * c * (1 + 3 + 1 + 1 + 1 + 8 + 4 + 1) + 4 * n * n * c + 4 * n * L * c + 4 * L * D * c

    enc, dec = W.encoder_layout(cfg), W.decoder_layout(cfg)
    mid_index = sum(b["attn"] for b in enc) + sum(b["attn"] for b in dec)
    tally = dict(total=0, behind=0, forked=False)

    def add(f, block=None):
        if block is not None and block in blocks:
            tally["forked"] = True
        tally["total"] += f
        if tally["forked"]:
            tally["behind"] += f

    blk = 0
    for b in enc:
        n = (h // b["ds"]) ** 2
        if b["kind"] == "conv_in":
            add(2 * n * 9 * 8 * b["cout"])
        elif b["kind"] == "down":
            add(2 * (n // 4) * 9 * b["cin"] * b["cout"])
        else:
            add(res(b["cin"], b["cout"], n))
            if b["attn"]:
                add(st(b["cout"], n), blk)
                blk += 1
    n, c = (h // enc[-1]["ds"]) ** 2, enc[-1]["cout"]
    add(res(c, c, n))
    add(st(c, n), mid_index)
    add(res(c, c, n))
    for b in dec:
        n = (h // b["ds"]) ** 2
        add(res(b["cin"], b["cout"], n))
        if b["attn"]:
            add(st(b["cout"], n), blk)
            blk += 1
        if b["up"]:
            add(2 * 4 * n * 9 * b["cout"] * b["cout"])
    return tally["total"], tally["behind"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3, help="timed passes per leg (each = one full sampling of the batch)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--precision", default="f16", choices=["f16", "bf16", "f16x2", "f32"])
    ap.add_argument("--out", default=None)
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
    mid = parse_pag_layers("mid", cfg)
    wide = parse_pag_layers(["down.block_2", "mid", "up.block_1"], cfg)
    state = {"off": (0.0, 0, 1), "zero": (0.0, mid, 1), "mid": (3.0, mid, 1), "mid_plain": (3.0, mid, 0), "wide": (3.0, wide, 1)}

    def use(leg):
        scale, mask, fork = state[leg]
        eng.set_option("pag_fork", fork)
        eng.set_pag(scale, mask)

    legs = tuple(state)
    times = {k: [] for k in legs}
    launches, pag_launches, fork_block, outs = {}, {}, {}, {}
    for leg in legs:   # warm-up, launch counts
        use(leg)
        n0, p0 = eng.stat("launches"), eng.stat("pag_launches")
        outs[leg] = eng.ddim_sample(**kw)
        torch.cuda.synchronize()
        launches[leg] = (eng.stat("launches") - n0) / args.steps
        pag_launches[leg] = (eng.stat("pag_launches") - p0) / args.steps
        fork_block[leg] = eng.stat("pag_fork_block")
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
    med = {k: statistics.median(v) for k, v in times.items()}
    spread_off = (max(times["off"]) - min(times["off"])) / med["off"]
    levels = []
    for ds, C in ((1, 320), (2, 640), (4, 1280), (8, 1280)):
        N = (h // ds) ** 2
        k_ms, c_ms = eng.bench_pag_identity(B, N, C, iters=50)
        moved = 2 * B * N * C * (4 if args.precision in ("f32", "f16x2") else 2)
        levels.append(dict(level=f"{h // ds}x{h // ds}", B=B, N=N, C=C, kernel_us=round(1e3 * k_ms, 2), copy_us=round(1e3 * c_ms, 2),
                           kernel_over_copy=round(k_ms / c_ms, 3), kernel_GBps=round(moved / (k_ms * 1e-3) / 1e9, 1)))
    # the forked part from shapes: B perturbed samples behind the fork, over the 2 B samples of the UNet alone (the ControlNet, about the
    # UNet's encoder and middle block again, is not counted in either)
    share = {}
    for leg, mask in (("mid", mid), ("wide", wide)):
        tot, behind = unet_flops(cfg, h, {j for j in range(32) if mask >> j & 1})
        share[leg] = round(100.0 * behind / (2 * tot), 2)
    res = dict(config=f"SD1.5 bs {B} {args.size}x{args.size} {args.steps}-step DDIM {args.precision}, CFG 7.5, random weights",
               images_per_s={k: round(B / med[k], 4) for k in legs},
               pass_s={k: [round(t, 4) for t in v] for k, v in times.items()},
               off_spread_pct=round(100 * spread_off, 3),
               cost_pct_vs_off={k: round(100.0 * (med[k] / med["off"] - 1.0), 3) for k in legs if k != "off"},
               fork_vs_plain_pct=round(100.0 * (med["mid"] / med["mid_plain"] - 1.0), 3),
               forked_flops_pct_of_unet_2B=share,
               launches_per_step=launches, pag_launches_per_step=pag_launches, fork_block=fork_block,
               zero_equals_off=bool(torch.equal(outs["zero"], outs["off"])),
               fork_equals_plain=bool(torch.equal(outs["mid"], outs["mid_plain"])),
               latent_relchange_vs_off={k: round(float((outs[k] - outs["off"]).abs().max() / outs["off"].abs().max()), 4) for k in ("mid", "wide")},
               identity_kernel_alone=levels)
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    eng.close()


if __name__ == "__main__":
    main()
