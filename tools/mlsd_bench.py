"""M-LSD line detector: Engine.mlsd("lines") on seeded random weights (weights.synth_mlsd_state_dict), one MI355X.

    python tools/mlsd_bench.py [--calls 7] [--warmup 3] [--timeout 300] [--out profiles/mlsd_bench.json]

For 8 x 512^2 and 1 x 512^2 pictures in f16 and bf16 (each leg a child process under its own time limit): the median wall time of the
whole call (CUDA uint8 tensor in, CUDA uint8 tensor out), and from a separate pass with option "profile" on the device time per
kernel family -- pointwise (every conv1x1 on the contraction path), depthwise (mlsd_dwconv_kernel), decoder (the conv3x3 of features.0
and of blocks 16..23 plus the upload / upsample / output kernels), decode + raster -- as the sum of the HIP-event brackets, per call.
For the depthwise kernel's three largest launches: bytes (one read of the input + one write of the output) over the bracket time against
the achievable HBM rate (6.3 TB/s measured of the 8 TB/s specification).  Prints one JSON line per leg and writes them all to --out.
"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ACHIEVABLE = 6.3e12
FAMILIES = {"pointwise": (1,), "depthwise": (8,), "decoder": (0, 3, 9), "decode_raster": (10,)}


def child(args):
    import dataclasses

    import torch

    from prompt_diffusion_amd import engine as E
    from prompt_diffusion_amd import weights as W

    B, S = args.batch, args.size
    e = E.Engine(dataclasses.replace(W.TINY, mlsd=True), device=0, precision=args.precision)
    e.load_mlsd_state_dict(W.synth_mlsd_state_dict(5))   # seeded random weights whose output is lively (about one pixel in nine is a peak)
    x = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    sync = torch.cuda.synchronize
    run = lambda: e.mlsd(x, 0.1, 0.1, what="lines")
    for _ in range(args.warmup):
        first = run()
    sync()
    l0 = e.stat("launches")
    ts = []
    for _ in range(args.calls):
        sync()
        t0 = time.perf_counter()
        run()
        sync()
        ts.append(time.perf_counter() - t0)
    launches = (e.stat("launches") - l0) // args.calls
    _, count = e.mlsd(x, 0.1, 0.1, what="segments")
    e.set_option("profile", 1)
    for _ in range(args.calls):
        run()
    fam = {}
    for name, klasses in FAMILIES.items():
        ms = n = 0
        for k in klasses:
            m, c, _ = e.profile_read(k)
            ms, n = ms + m, n + c
        fam[name] = dict(ms_per_call=round(ms / args.calls, 4), brackets_per_call=n / args.calls)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "prof.csv")
        e.profile_dump(path)
        rows = [r for r in csv.DictReader(open(path)) if int(r["klass"]) == 8]
    e.set_option("profile", 0)
    es = 2
    shapes = {}
    for r in rows:
        stride = int(r["taps"]) - 90
        key = (int(r["M"]), int(r["N"]), stride)
        shapes.setdefault(key, []).append(float(r["ms"]))
    table = []
    for (M, C, stride), ms in shapes.items():
        nbytes = (M * stride * stride + M) * C * es
        t = statistics.median(ms)
        table.append(dict(out_pixels=M, channels=C, stride=stride, launches_per_call=len(ms) // args.calls, bytes=nbytes, median_ms=round(t, 4),
                          bytes_per_s=round(nbytes / (t * 1e-3)) if t > 0 else None,
                          of_achievable_hbm=round(nbytes / (t * 1e-3) / HBM_ACHIEVABLE, 3) if t > 0 else None))
    table.sort(key=lambda r: -r["bytes"])
    dev_ms = sum(f["ms_per_call"] for f in fam.values())
    wall = statistics.median(ts)
    print(json.dumps(dict(config=f"M-LSD lines bs {B} {S}x{S} {args.precision}", gpu=torch.cuda.get_device_name(0), call_ms=round(1e3 * wall, 3),
                          call_ms_all=[round(1e3 * t, 3) for t in ts], launches_per_call=int(launches), segments_per_image=[int(c) for c in count.cpu()],
                          families=fam, bracketed_device_ms=round(dev_ms, 4), wall_minus_device_ms=round(1e3 * wall - dev_ms, 4),
                          us_per_launch_wall=round(1e6 * wall / max(1, int(launches)), 2), depthwise_largest=table[:3],
                          lines_fraction=round(float((first == 255).float().mean()), 4))))
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlsd_bench.json"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    legs = []
    for prec in ("f16", "bf16"):
        for B in (8, 1):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--batch", str(B), "--size", str(args.size), "--precision", prec,
                   "--calls", str(args.calls), "--warmup", str(args.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            if r.returncode != 0:          # nothing more is started on the GPU after a failed leg
                sys.stderr.write(r.stdout + r.stderr)
                sys.exit(f"mlsd_bench: the {prec} batch-{B} leg ended with status {r.returncode}")
            line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
            print(line, flush=True)
            legs.append(json.loads(line))
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/mlsd_bench.py", hbm_achievable_bytes_per_s=HBM_ACHIEVABLE, legs=legs), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
