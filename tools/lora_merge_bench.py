"""Time of a LoRA merge on the device (pd_lora_set_scales: merge kernels + LayerNorm refold + synchronise) over every SD1.5 UNet
attention / feed-forward / proj matrix, against re-uploading the same host-merged tensors through pd_load_weights, and the
device memory of the base copies.  Prints one JSON line per rank.

    python tools/lora_merge_bench.py [--ranks 8 64 128] [--reps 10] [--precision f16] [--out FILE]

With --forms it times, in the same process and over the same matrices, pd_lora_set_scales for a plain rank-64 pair, a LoHa adapter
(two rank-32 products), a LoKr adapter (w1 [8, 8]) and a rank-64 pair under a DoRA magnitude: medians of --reps merges alternating
two scales, each with its ratio to the plain merge and to the host-merge-and-re-upload time of that run.

    python tools/lora_merge_bench.py --forms [--forms-out profiles/lora_forms_bench.json]
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


def form_factors(kind, shape, g):
    """operands of Engine.lora_add_ex for one bench adapter on a tensor of `shape`"""
    n, k = shape[0], int(np.prod(shape[1:]))
    f = lambda *s: g.standard_normal(s, dtype=np.float32) * np.float32(0.01)
    if kind == "loha":
        return dict(kind="hada", up=f(n, 32), down=f(32, k), up2=f(n, 32), down2=f(32, k) * np.float32(100))
    if kind == "lokr":
        return dict(kind="kron", up=f(8, 8), down=f(n // 8, shape[1] // 8, *shape[2:]))
    return dict(kind="pair", up=f(n, 64), down=f(64, k), magnitude=np.abs(f(n)) * np.float32(100) if kind == "lora+dora" else None)


def bench_forms(e, names, shapes, reps, precision):
    rows = []
    for kind in ("lora", "loha", "lokr", "lora+dora"):
        g = np.random.default_rng(len(kind))
        for n in names:
            e.lora_add_ex(0, n, **form_factors(kind, shapes[n], g))
        e.lora_set_scales([1.0])   # warm-up
        e.lora_set_scales([0.5])
        t = []
        for i in range(reps):
            t0 = time.perf_counter()
            e.lora_set_scales([1.0 if i % 2 else 0.75])
            t.append((time.perf_counter() - t0) * 1e3)
        row = dict(form=kind, precision=precision, targets=len(names), merge_ms_median=float(np.median(t)), merge_ms_min=float(np.min(t)),
                   adapter_bytes=int(e.stat("lora_bytes") - e.stat("lora_base_bytes")))
        if kind == "lora":           # the re-upload column: the same host-merged tensors through pd_load_weights
            merged = {n: e.read_weight(n) for n in names}
            e.lora_remove(-1)
            up = []
            for _ in range(2):
                t0 = time.perf_counter()
                for n in names:
                    e.load_tensor(n, merged[n])
                e.synchronize()
                up.append((time.perf_counter() - t0) * 1e3)
            reupload = float(np.min(up))
            e.init_random_weights(1)
        else:
            e.lora_remove(-1)
        row["reupload_ms"] = reupload
        row["ratio_to_plain"] = row["merge_ms_median"] / rows[0]["merge_ms_median"] if rows else 1.0
        row["ratio_to_reupload"] = row["merge_ms_median"] / reupload
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forms", action="store_true", help="time LoHa / LoKr / LoRA+DoRA next to the plain rank-64 merge instead")
    ap.add_argument("--forms-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                         "lora_forms_bench.json"))
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
    if a.forms:
        rows = bench_forms(e, names, shapes, a.reps, a.precision)
        e.close()
        os.makedirs(os.path.dirname(os.path.abspath(a.forms_out)), exist_ok=True)
        with open(a.forms_out, "w") as f:
            json.dump(rows, f, indent=1)
        return
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
