"""Times SD3's VAE on the engine at SD3_MEDIUM_VAE with random weights, with the mid-block attention on the single-head flash kernel
(option vae_flash 1) and on the materialised path (0):

  attention alone  softmax(q k^T C^-0.5) v at C = 512, N = 4096 and N = 16384 (pd_bench_vae_attention: back-to-back launches between two events)
  decode 1024^2    latents [B, 16, 128, 128] -> images, B = 1 and 2
  encode 1024^2    images [B, 3, 1024, 1024] -> latents (mode "mean"), B = 1 and 3

    python tools/sd3_vae_bench.py [--precisions bf16,f16] [--size 1024] [--out profiles/sd3_vae_bench.json]

Method: inputs and outputs live on the device; every engine call ends in a stream synchronise, so a host clock around it times the device
work plus its launches.  Each (case, path) is warmed up, then the two paths are timed in ALTERNATING order, call by call, in one process
on one box; the figure is the median.  arena_mib is the engine's side workspace (stat "side_workspace_bytes") after the call: it never shrinks, so every
(precision, path) pair runs on an engine of its own.  Compare numbers from one run only."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prompt_diffusion_amd import sd3  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precisions", default="bf16,f16")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sd3_vae_bench: no GPU; this tool only measures on one")
    vc = sd3.SD3_MEDIUM_VAE
    net = sd3.SD3Config(heads=2, head_dim=64, layers=1, cn_layers=0, joint_dim=96, pooled_dim=40, pos_embed_max_size=16)
    rows = []

    def emit(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    for prec in a.precisions.split(","):
        engs = {}
        for flash in (1, 0):
            e = sd3.SD3Engine(net, precision=prec)
            e.configure_vae(vc)
            e.init_random_weights(1)
            e.base.set_option("vae_flash", flash)
            engs[flash] = e
        # ---- the attention product alone
        for N in (4096, 16384):
            ms, sb = {1: [], 0: []}, {}
            for rep in range(3):
                for flash in ((1, 0) if rep % 2 == 0 else (0, 1)):
                    t, b = C.c_float(), C.c_int64()
                    eb = engs[flash].base
                    eb._check(eb.lib.pd_bench_vae_attention(eb._h, 1, N, 512, flash, 5, C.byref(t), C.byref(b)))
                    ms[flash].append(float(t.value))
                    sb[flash] = int(b.value)
            for flash in (1, 0):
                emit(case="attention", precision=prec, B=1, N=N, C=512, vae_flash=flash, ms=round(statistics.median(ms[flash]), 3),
                     score_mib=round(sb[flash] / 2 ** 20, 1), tflops=round(4.0 * N * N * 512 / statistics.median(ms[flash]) / 1e9, 1))
        # ---- whole decode / encode
        S = a.size
        g = torch.Generator(device="cuda").manual_seed(0)
        for case, B in (("decode", 1), ("decode", 2), ("encode", 1), ("encode", 3)):
            if case == "decode":
                x = torch.randn((B, vc.z_channels, S // 8, S // 8), device="cuda", generator=g)
                fn = lambda e: e.vae_decode(x)
            else:
                x = torch.rand((B, 3, S, S), device="cuda", generator=g) * 2 - 1
                fn = lambda e: e.vae_encode(x, mode="mean")
            ts = {1: [], 0: []}
            for flash in (1, 0):
                fn(engs[flash])          # warm-up: sizes the workspace
                fn(engs[flash])
            for i in range(a.calls):
                for flash in ((1, 0) if i % 2 == 0 else (0, 1)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(engs[flash])      # ends in a stream synchronise
                    ts[flash].append((time.perf_counter() - t0) * 1e3)
            for flash in (1, 0):
                emit(case=case, precision=prec, B=B, size=S, vae_flash=flash, ms=round(statistics.median(ts[flash]), 2), calls=len(ts[flash]),
                     flash_launches=engs[flash].base.stat("vae_flash_launches"), arena_mib=round(engs[flash].base.stat("side_workspace_bytes") / 2 ** 20, 1))
        for e in engs.values():
            e.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
