"""Times tiled against untiled VAE calls (Engine.set_vae_tiling) with random weights, in one process on one box:

  SD1.5 first stage  decode and encode at 512^2, 1024^2, 1536^2 and 2048^2 (tile_latent 64: 512^2 is not tiled at all)
  SD3's VAE          decode and encode at 1024^2 (not tiled at tile_latent 128) and 2048^2

    python tools/vae_tiling_bench.py [--precisions f16,bf16] [--calls 5] [--out profiles/vae_tiling_bench.json]

Per (VAE, precision) there is one untiled engine and one tiled engine per tile_batch in {1, 4, 16, all}: the side workspace (stat
"side_workspace_bytes") never shrinks, so an engine of its own per variant, walked through the sizes in ascending order, is what makes
workspace_mib the need of that size.  Method: inputs and outputs live on the device; every engine call ends in a stream synchronise,
so a host clock around it times the device work plus its launches.  Each variant is warmed up twice, then the variants are timed
call by call in rotating order; the figure is the median (ms_min / ms_max: the spread of those calls; `tiles` is 0 where the variant
or the size is not tiled).  `attention` is the path the untiled call's mid-block attention took (stat
"vae_flash_launches").  A variant that fails (out of memory at the largest sizes) is recorded with its error.  Compare numbers from one
run only."""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prompt_diffusion_amd import engine as E  # noqa: E402
from prompt_diffusion_amd import sd3  # noqa: E402
from prompt_diffusion_amd import weights as W  # noqa: E402

BATCHES = (("1", 1), ("4", 4), ("16", 16), ("all", 1 << 20))


def make(vae, prec):
    if vae == "sd15":
        e = E.Engine(dataclasses.replace(W.SD15, vae_encoder=True), precision=prec)
        e.init_random_weights(1)
        return e, e
    net = sd3.SD3Config(heads=2, head_dim=64, layers=1, cn_layers=0, joint_dim=96, pooled_dim=40, pos_embed_max_size=16)
    e = sd3.SD3Engine(net, precision=prec)
    e.configure_vae(sd3.SD3_MEDIUM_VAE)
    e.init_random_weights(1)
    return e, e.base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precisions", default="f16,bf16")
    ap.add_argument("--vaes", default="sd15,sd3")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--max-size", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("vae_tiling_bench: no GPU; this tool only measures on one")
    rows = []

    def emit(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)
                f.write("\n")

    g = torch.Generator(device="cuda").manual_seed(0)
    for vae in a.vaes.split(","):
        sizes = [s for s in ((512, 1024, 1536, 2048) if vae == "sd15" else (1024, 2048)) if s <= a.max_size]
        zc = 4 if vae == "sd15" else sd3.SD3_MEDIUM_VAE.z_channels
        for prec in a.precisions.split(","):
            engs = {"untiled": make(vae, prec)}
            for name, tb in BATCHES:
                engs["tiled_" + name] = make(vae, prec)
                engs["tiled_" + name][0].set_vae_tiling(True, tile_batch=tb)
            dead = set()
            for S in sizes:
                for case in ("decode", "encode"):
                    if case == "decode":
                        x = torch.randn((1, zc, S // 8, S // 8), device="cuda", generator=g)
                        fn = lambda e: e.vae_decode(x)
                        plan = engs["tiled_1"][0].vae_tile_plan(S // 8, S // 8)
                    else:
                        x = torch.rand((1, 3, S, S), device="cuda", generator=g) * 2 - 1
                        fn = lambda e: e.vae_encode(x, mode="mean")
                        plan = engs["tiled_1"][0].vae_tile_plan(S, S, encode=True)
                    ts, flash, err = {k: [] for k in engs}, {}, {}
                    for k, (e, base) in engs.items():
                        if k in dead:
                            continue
                        try:
                            f0 = base.stat("vae_flash_launches")
                            fn(e)            # warm-up: sizes the workspace
                            fn(e)
                            flash[k] = base.stat("vae_flash_launches") > f0
                        except E.PdError as ex:
                            err[k] = str(ex)
                            dead.add(k)      # (a failed allocation: leave this engine alone for the larger sizes too)
                    live = [k for k in engs if k not in dead]
                    for i in range(a.calls):
                        for k in live[i % len(live):] + live[:i % len(live)]:
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            fn(engs[k][0])   # ends in a stream synchronise
                            ts[k].append((time.perf_counter() - t0) * 1e3)
                    for k, (e, base) in engs.items():
                        row = dict(vae=vae, precision=prec, case=case, size=S, variant=k, tiles=0 if k == "untiled" else plan.rows * plan.cols)
                        if k in err or k in dead:
                            emit(**row, error=err.get(k, "skipped after an earlier failure"))
                            continue
                        if k == "untiled":
                            row["attention"] = "flash" if flash[k] else "materialised"
                        emit(**row, ms=round(statistics.median(ts[k]), 2), ms_min=round(min(ts[k]), 2), ms_max=round(max(ts[k]), 2), calls=len(ts[k]),
                             workspace_mib=round(base.stat("side_workspace_bytes") / 2 ** 20, 1))
                    del x
            for e, _ in engs.values():
                e.close()


if __name__ == "__main__":
    main()
