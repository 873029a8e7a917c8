"""HED edge detector: Engine.hed against torch eager running the same network (tests/hed_ref.py) on the same GPU.

    python tools/hed_bench.py [--batch 8] [--size 512] [--precision f16] [--warmup 3] [--runs 10] [--timeout 600]
    python tools/hed_bench.py --stats      # one rocprofv3 --kernel-trace --stats run of three Engine.hed calls: per-kernel split

The timed legs alternate call by call (engine, torch, engine, ..) so clock and thermal drift hit both alike; device tensors in and
out, medians of `runs` calls after `warmup` untimed ones each.  Every GPU step is a child process under its own time limit.
Prints one JSON line.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(args):
    import dataclasses

    import torch

    from prompt_diffusion_amd import engine as E
    from prompt_diffusion_amd import weights as W
    from tests import hed_ref

    dev = torch.device("cuda", 0)
    sd = W.synth_hed_state_dict()
    eng = E.Engine(dataclasses.replace(W.TINY, hed=True), device=0, precision=args.precision)
    eng.load_hed_state_dict(sd)
    x = torch.rand((args.batch, 3, args.size, args.size), generator=torch.Generator(device=dev).manual_seed(7), device=dev)
    if args.mode == "stats":   # under rocprofv3: the engine alone
        for _ in range(3):
            eng.hed(x)
        torch.cuda.synchronize()
        return
    tdt = {"f16": torch.float16, "bf16": torch.bfloat16}.get(args.precision, torch.float32)
    tsd = {k: torch.from_numpy(v).to(device=dev, dtype=tdt) for k, v in sd.items()}

    def run_engine():
        return eng.hed(x)

    def run_torch():
        with torch.no_grad():
            return hed_ref.forward_bgr(tsd, x.flip(1).to(tdt))[1].float()

    legs = {"engine": run_engine, "torch": run_torch}
    outs = {}
    for name, fn in legs.items():
        for _ in range(args.warmup):
            outs[name] = fn()
        torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.runs):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    diff = float((outs["engine"] - outs["torch"]).abs().max())
    print(json.dumps(dict(config=f"HED bs {args.batch} {args.size}x{args.size} {args.precision}", gpu=torch.cuda.get_device_name(0),
                          engine_ms=round(1e3 * statistics.median(times["engine"]), 3), torch_eager_ms=round(1e3 * statistics.median(times["torch"]), 3),
                          engine_ms_all=[round(1e3 * t, 3) for t in times["engine"]], torch_ms_all=[round(1e3 * t, 3) for t in times["torch"]],
                          edge_max_abs_diff=round(diff, 5))))
    eng.close()


def kernel_table(d):
    """name, calls, total ms, share from rocprofv3's *_kernel_stats.csv"""
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((r["Name"], int(r["Calls"]), float(r["TotalDurationNs"]) / 1e6))
    tot = sum(r[2] for r in rows) or 1.0
    return [r + (100.0 * r[2] / tot,) for r in sorted(rows, key=lambda r: -r[2])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--precision", default="f16", choices=["f16", "bf16", "f16x2", "f32"])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=600, help="seconds each GPU step may take")
    ap.add_argument("--stats", action="store_true", help="per-kernel split from one rocprofv3 --kernel-trace --stats run")
    ap.add_argument("--mode", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.mode:
        return child(args)
    me = [sys.executable, os.path.abspath(__file__), "--batch", str(args.batch), "--size", str(args.size), "--precision", args.precision,
          "--warmup", str(args.warmup), "--runs", str(args.runs)]
    if not args.stats:
        r = subprocess.run(["timeout", "-k", "10", str(args.timeout)] + me + ["--mode", "time"])
        sys.exit(r.returncode)
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["timeout", "-k", "10", str(args.timeout), "rocprofv3", "--kernel-trace", "--stats", "-d", d, "--output-format", "csv", "--"] + me + ["--mode", "stats"], capture_output=True, text=True)
        if r.returncode:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            sys.exit(r.returncode)
        for name, calls, ms, pct in kernel_table(d):
            print(f"{ms / 3:9.3f} ms/call-of-hed {calls:4d} launches {pct:6.2f} %  {name[:120]}")


if __name__ == "__main__":
    main()
