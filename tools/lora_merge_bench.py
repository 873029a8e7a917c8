"""Time of a LoRA merge on the device (pd_lora_set_scales: merge kernels + LayerNorm refold + synchronise) over every SD1.5 UNet
attention / feed-forward / proj matrix, against re-uploading the same host-merged tensors through pd_load_weights, and the
device memory of the base copies.  Prints one JSON line per rank.

    python tools/lora_merge_bench.py [--ranks 8 64 128] [--reps 10] [--precision f16] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from prompt_diffusion_amd import engine as E  # noqa: E402
from prompt_diffusion_amd import lora as L  # noqa: E402
from prompt_diffusion_amd import weights as W  # noqa: E402


def targets(cfg):
    return [n for d, n in L.unet_module_map(cfg).items() if ".attentions." in d]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, nargs="+", default=[8, 64, 128])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = W.SD15
    e = E.Engine(cfg, precision=a.precision)
    e.init_random_weights(1)
    shapes = dict(e.param_names())
    names = targets(cfg)
    n_params = sum(int(np.prod(shapes[n])) for n in names)
    rows = []
    for r in a.ranks:
        g = np.random.default_rng(r)
        for n in names:
            s = shapes[n]
            up = g.standard_normal((s[0], r), dtype=np.float32) * np.float32(0.01)
            down = g.standard_normal((r,) + tuple(s[1:]), dtype=np.float32) * np.float32(0.01)
            e.lora_add(0, n, up, down)
        e.lora_set_scales([1.0])   # warm-up: first launch of every shape, LayerNorm fold buffers
        e.lora_set_scales([0.5])
        t = []
        for i in range(a.reps):
            t0 = time.perf_counter()
            e.lora_set_scales([1.0 if i % 2 else 0.75])
            t.append((time.perf_counter() - t0) * 1e3)
        merged = {n: e.read_weight(n) for n in names}
        base_bytes, all_bytes = e.stat("lora_base_bytes"), e.stat("lora_bytes")
        e.lora_remove(-1)
        up_plain = []
        for _ in range(2):
            t0 = time.perf_counter()
            for n in names:
                e.load_tensor(n, merged[n])
            e.synchronize()
            up_plain.append((time.perf_counter() - t0) * 1e3)
        flops = 2.0 * r * n_params
        row = dict(rank=r, precision=a.precision, targets=len(names), params=n_params, merge_ms_median=float(np.median(t)),
                   merge_ms_min=float(np.min(t)), reupload_ms=float(np.min(up_plain)), base_copy_bytes=int(base_bytes),
                   adapter_bytes=int(all_bytes - base_bytes), merge_gflop=flops / 1e9)
        rows.append(row)
        print(json.dumps(row), flush=True)
        e.init_random_weights(1)
    e.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
