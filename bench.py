#!/usr/bin/env python3
"""bench.py -- headline benchmark of the Prompt-Diffusion DDIM hot path on MI355X.

Metric (BASELINE.json): images/sec @ 512x512, 50-step DDIM, bs=8 (per GPU; weak scaling:
N GPUs sample 8*N images, batch-sharded, one RCCL all-gather of the final latents per pass).
A "step" (--steps K) is one full pass of the hot path over one batch: pd_ddim_sample of 8 images =
50 denoising steps x (ControlNet + UNet on the CFG-doubled batch 16) + CFG + DDIM update, with every
input already resident in HBM (torch CUDA tensors handed over as device pointers).  Weights are
random-initialised on the device (no checkpoint exists offline), inputs synthetic.

Usage:  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
        python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
`python bench.py --gpus N` without a torchrun environment launches that second line itself, as a CHILD process and
before anything touches the GPU, and relays the child's JSON line.  Prints ONE JSON line on rank 0.
A plain run does only what the headline needs: set-up, W warm-up passes, the K timed passes, the dump, the JSON line.
--full adds, after the timed passes, everything that takes runs of its own: the rate with option cfg_share off, the profiled
pass behind `roofline`, the VAE decode, the `parity` leg against tests/golden/, the f16x2 mode, the SD3 leg and the CPU
baseline (each of which a --no-* flag skips).
--dump-outputs DIR writes what the last timed step returned (the final latents of every image, float32) as DIR/latents.npy;
the weights and inputs are seeded, so two builds run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0   # dense bf16 MFMA, MI355X_MICROARCH.md
PEAK_F32_TFLOPS = 157.3
# algorithmic FLOPs per forward-sample at latent 64x64 with loop invariants hoisted
GF_PER_FWD_SAMPLE_64 = 1067.5


def shared_front_gf(h: int, w: int, fused_tail: bool = True) -> float:
    """GF per CFG PAIR that option "cfg_share" does not execute (the layers in front of the first cross-attention run once for the
    pair instead of twice; pd_engine::forward_eps): conv_in, the first ResBlock's two 3x3 convs, proj_in, to_q/k/v and the N x N
    self-attention of the first SpatialTransformer, in the UNet and in the ControlNet, plus the ControlNet's first zero conv.  (With
    the per-layer transformer path attn1.to_out and attn2.to_q are shared too; the fused tail kernel recomputes them per half.)"""
    n, c = h * w, 320
    conv_in = 2 * n * c * 9 * 4
    res = 2 * (2 * n * c * 9 * c)
    lin = 2 * n * c * c
    attn = 4 * 8 * n * n * (c // 8)
    per_net = conv_in + res + 4 * lin + attn + (0 if fused_tail else 2 * lin)
    return (2 * per_net + lin) / 1e9


def cpu_baseline(ddim_steps: int):
    """The oracle (NumPy restatement, kind 'port') timed on the host cores on a bounded sample of the same
    workload: ONE denoising step of ONE 512x512 image (CFG pair, latent 64x64); images/sec is
    extrapolated as 1 / (ddim_steps * t_step)."""
    import numpy as np
    from oracle import pd_oracle as O
    from prompt_diffusion_amd import weights as W
    cfg = W.SD15
    sd = W.synth_state_dict(cfg)
    lay = O.make_layouts(cfg, W)
    inp = W.synth_inputs(cfg, 1, 64, 64)
    cond = dict(c_crossattn=inp["ctx_cond"], example_pair=inp["pair"], query=inp["query"])
    unc = dict(c_crossattn=inp["ctx_uncond"], example_pair=inp["pair"], query=inp["query"])
    sched = O.make_schedule(ddim_steps)
    t0 = time.time()
    O.p_sample_ddim(sd, cfg, lay, sched, inp["x_T"], cond, unc, ddim_steps - 1, int(sched["ddim_timesteps"][-1]), 7.5)
    dt = time.time() - t0
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    return dict(value=1.0 / (ddim_steps * dt), unit="images/sec", cores=cores, kind="port",
                sample=f"1 of {ddim_steps} DDIM steps of one 512x512 image (CFG pair) = {dt:.1f} s on the host cores, "
                       f"NumPy/OpenBLAS fp32; extrapolated x{ddim_steps}")


def parity_leg(E, W, precision, stream_f32, device):
    """The second half of BASELINE's metric: per-step latent error against the reference's own CPU trajectories
    (tests/golden/, made by tests/golden/make_golden.py from the reference project), computed in this run with the seeded
    synthetic weights those fixtures were made with.  `per_step_relerr`: 50-step schedule (the metric's schedule) --
    the engine gets the reference's x_i and must reproduce x_{i+1}; max over the sampled steps of max|dx| / max|x_ref|."""
    import numpy as np
    gdir = os.path.join(ROOT, "tests", "golden")
    f50, f5 = os.path.join(gdir, "net_sd15_b1_32x32_s50.npz"), os.path.join(gdir, "net_sd15_b1_32x32_s5.npz")
    if not os.path.exists(f50):
        return None
    cfg = W.SD15
    e = E.Engine(cfg, device=device, precision=precision, stream_f32=stream_f32)
    for n, a in W.iter_synth(cfg):
        e.load_tensor(n, a)
    g = np.load(f50)
    B, h, w, S = int(g["B"]), int(g["h"]), int(g["w"]), int(g["S"])
    inp = W.synth_inputs(cfg, B, h, w)
    kw = dict(x_T=inp["x_T"], ctx_cond=inp["ctx_cond"], ctx_uncond=inp["ctx_uncond"], pair=inp["pair"], query=inp["query"],
              steps=S, cfg_scale=float(g["cfg_scale"]))
    ref = g["x_inter"]
    steps = list(range(S))   # every step of the schedule
    e.sample_begin(**kw)
    rel, mabs = [], []
    for i in steps:
        e.sample_set_latents(ref[i])
        e.sample_step(i)
        d = np.abs(e.sample_get() - ref[i + 1]).max()
        rel.append(float(d / np.abs(ref[i + 1]).max()))
        mabs.append(float(d))
    e.sample_end()
    out = {"per_step_relerr": max(rel), "per_step_max_abs_err": max(mabs), "steps_checked": len(steps), "parity_ok": bool(max(rel) <= 1e-3),
           "schedule": "50-step DDIM, CFG 7.5, SD1.5 256x256 bs 1 (tests/golden/net_sd15_b1_32x32_s50.npz: the reference's CPU trajectory)",
           "bound": 1e-3, "mode": precision}
    if os.path.exists(f5):   # BASELINE config #1: the 5-step trajectory, whole loop from x_T
        g5 = np.load(f5)
        o5, inter = e.ddim_sample(x_T=inp["x_T"], ctx_cond=inp["ctx_cond"], ctx_uncond=inp["ctx_uncond"], pair=inp["pair"],
                                  query=inp["query"], steps=int(g5["S"]), cfg_scale=float(g5["cfg_scale"]), return_intermediates=True)
        out["config1_per_step_relerr"] = max(float(np.abs(inter[i] - g5["x_inter"][i]).max() / np.abs(g5["x_inter"][i]).max())
                                             for i in range(1, int(g5["S"]) + 1))
        out["config1"] = "#1: 256x256, 5 DDIM steps, bs 1 (8x larger eps coefficient per step than the 50-step schedule)"
        out["config1_parity_ok"] = bool(out["config1_per_step_relerr"] <= 1e-3)
        # no 2-byte mode can meet 1e-3 on this schedule: rounding the WEIGHTS alone to fp16 already costs 8.5e-4 per step
        # (error budget); the conforming mode for config #1 is f16x2 (<= 5e-6, reported under "f16x2")
        out["config1_conforming_mode"] = "f16x2" if precision in ("f16", "bf16") else precision
    e.close()
    return out


def spawn_ranks(n: int) -> int:
    """`python bench.py --gpus N` outside torchrun: start the N-rank job as a child (one process per GPU, RCCL) and relay
    its output.  Nothing in this process has touched the GPU (no torch import yet), so starting children is safe."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.run(cmd, env=env).returncode


def sd3_leg(precision, device):
    """Context only (not the metric): the SD3 / MMDiT variant of the path (BASELINE config #5) at
    SD3-medium size + a 6-block ControlNet, 1024x1024 (4096 image + 333 context tokens), CFG, random-init weights: 10 Euler
    steps timed after a warm-up pass, without and with e4m3 operands on the AdaLN-fed projections ("fp8 MFMA")."""
    import torch
    from prompt_diffusion_amd import sd3
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from sd3_bench import step_flops
    out = {"workload": "SD3-medium MMDiT + 6-block Prompt-Diffusion ControlNet, 1024x1024, CFG 7 (forward batch 2), per Euler step",
           "parity": "unpinned (diffusers absent offline; oracle/sd3_oracle.py)"}
    cfg = sd3.SD3Config(pos_embed_max_size=96)
    g = torch.Generator(device="cuda").manual_seed(0)
    f = lambda *s: torch.randn(*s, device="cuda", generator=g)
    x, cond, pair = f(1, 16, 128, 128), f(1, 16, 128, 128), f(1, 16, 128, 128)
    ctx, nctx, pool, npool = f(1, 333, cfg.joint_dim), f(1, 333, cfg.joint_dim), f(1, cfg.pooled_dim), f(1, cfg.pooled_dim)
    fl = step_flops(cfg, 2, 4096, 333)
    steps = 10
    try:
        for name, fp8 in (("f16" if precision == "f16" else precision, False), (precision + "+fp8", True)):
            e = sd3.SD3Engine(cfg, device=device, precision=precision, fp8=fp8)
            e.init_random_weights(7)
            run = lambda: e.sample(x, ctx, pool, nctx, npool, control_latents=cond, pair_latents=pair, num_inference_steps=steps,
                                   guidance_scale=7.0)
            o = run()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            o = run()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert torch.isfinite(o).all()
            out[name] = {"ms_per_step": 1e3 * dt / steps, "s_per_28_step_image": 28 * dt / steps, "path_tflops_per_s": fl * steps / dt / 1e12}
            e.close()
    except Exception as ex:   # noqa: BLE001 - context only
        out["error"] = str(ex)
    return out


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(d: str, **arrays) -> None:
    """Write each array as d/<name>.npy in float32.  An array over its share of DUMP_MAX_BYTES is written as a fixed sample
    instead: the elements at seeded random flat indices, in index order (d/<name>_index.npy holds the indices, float64).
    A directory this creates gets a .gitignore of its own, so that a dump inside a checkout leaves `git status` clean."""
    import numpy as np
    cap = DUMP_MAX_BYTES // max(len(arrays), 1) // 12    # elements per array: float32 values + float64 indices
    if not os.path.isdir(d):
        os.makedirs(d)
        with open(os.path.join(d, ".gitignore"), "w") as f:
            f.write("*\n")
    for name, a in arrays.items():
        if hasattr(a, "detach"):
            a = a.detach().float().cpu().numpy()
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.size > cap:
            idx = np.sort(np.random.default_rng(0).choice(a.size, cap, replace=False))
            np.save(os.path.join(d, name + "_index.npy"), idx.astype(np.float64))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(d, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2, help="timed passes (each = one 50-step sampling of the batch)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed passes, write the latents the last one returned to DIR/latents.npy (float32)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=8, help="images per GPU")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--precision", default="f16", choices=["f16", "bf16", "f16x2", "f32"],
                    help="engine mode; f16 (default) is the reference's own GPU dtype (README.md:44-45)")
    ap.add_argument("--stream-f32", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run the legs that take runs of their own (cfg_share-off rate, profiled roofline pass, "
                         "VAE decode, parity, f16x2 mode, SD3 leg, CPU baseline); the --no-* flags below skip single legs of --full")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--no-f32", "--no-extra-modes", dest="no_f32", action="store_true",
                    help="skip the extra measurement of the f16x2 mode (fp32-class results) on the same workload")
    ap.add_argument("--no-parity", action="store_true", help="skip the per-step latent error leg")
    ap.add_argument("--no-sd3", action="store_true", help="skip the SD3 / MMDiT leg (SURVEY N4 / BASELINE config #5, context only)")
    ap.add_argument("--engine-comm", action="store_true", help="N > 1: gather the final latents over the RCCL communicator the engine owns (pd_comm_*) instead of torch.distributed")
    ap.add_argument("--opt", action="append", default=[], help="engine tuning option key=int (experiments)")
    ap.add_argument("--no-cfg-share", action="store_true",
                    help="run the layers in front of the first cross-attention on the doubled batch like the reference does (option cfg_share 0)")
    ap.add_argument("--single-stream", action="store_true",
                    help="serialise ControlNet and UNet on one stream in every pass (used for the committed rocprof summary, so\n"
                         "that per-kernel durations are not stretched by the concurrent kernel of the other stream)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(spawn_ranks(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch with --nproc-per-node {args.gpus}")

    import torch
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the pdengine hot path has no CPU fallback")
    # PD_BENCH_REHEARSE=1: rehearse the N > 1 control flow on a single-GPU box (every rank on device 0, gloo instead of RCCL)
    rehearse = os.environ.get("PD_BENCH_REHEARSE") == "1"
    if rehearse:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearse:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        assert dist.get_world_size() == args.gpus

    from prompt_diffusion_amd import engine as E
    from prompt_diffusion_amd import weights as W
    from prompt_diffusion_amd.dist import shard_batch, all_gather_latents

    cfg = W.SD15
    B, S = args.batch, args.ddim_steps
    h = w = args.size // 8
    eng = E.Engine(cfg, device=local, precision=args.precision, stream_f32=args.stream_f32)
    eng.init_random_weights(1234 + rank)
    if args.single_stream:
        eng.set_option("two_streams", 0)
    if args.no_cfg_share:
        eng.set_option("cfg_share", 0)
    for o in args.opt:
        k, v = o.split("=")
        eng.set_option(k, int(v))

    gen = torch.Generator(device=dev).manual_seed(2023 + rank)
    x_T = torch.randn((B, 4, h, w), generator=gen, device=dev)
    ctx_c = torch.randn((B, cfg.context_len, cfg.context_dim), generator=gen, device=dev)
    ctx_u = torch.randn((B, cfg.context_len, cfg.context_dim), generator=gen, device=dev)
    pair = torch.rand((B, 6, 8 * h, 8 * w), generator=gen, device=dev) * 2 - 1
    query = torch.rand((B, 3, 8 * h, 8 * w), generator=gen, device=dev) * 2 - 1
    kw = dict(x_T=x_T, ctx_cond=ctx_c, ctx_uncond=ctx_u, pair=pair, query=query, steps=S, cfg_scale=7.5, eta=0.0)

    engine_comm = world > 1 and args.engine_comm and not rehearse
    if engine_comm:
        # the gather over the communicator the ENGINE owns (pd_comm_*: what a host without torch would use); the 128-byte id
        # travels over the process group that the barrier and the timing exchange use anyway
        box = [eng.comm_new_id() if rank == 0 else None]
        dist.broadcast_object_list(box, src=0)
        eng.comm_init(box[0], world, rank)

    def one_pass():
        lat = eng.ddim_sample(**kw)          # blocking: stream-synchronised on return
        if engine_comm:
            lat = eng.comm_all_gather(lat)
        elif world > 1:
            lat = all_gather_latents(lat, sizes=[B] * world)    # the path's only exchange: ONE all-gather of the final latents over RCCL/xGMI
        return lat

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        one_pass()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = one_pass()
    barrier()
    dt = time.perf_counter() - t0
    rank_ms = [1e3 * dt / args.steps]
    if world > 1:
        # MAX over ranks is the job's time; every rank's own time travels along so that a first real multi-GPU run diagnoses itself
        tall = [torch.zeros(1, device="cpu" if rehearse else dev, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(tall, torch.tensor([dt], device="cpu" if rehearse else dev, dtype=torch.float64))
        rank_ms = [1e3 * float(t.item()) / args.steps for t in tall]
        dt = max(float(t.item()) for t in tall)
    assert torch.isfinite(out).all(), "non-finite latents"
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, latents=out)
    images = world * B * args.steps
    value = images / dt

    result = {
        "metric": "images/sec @ 512x512, 50-step DDIM, bs=8", "value": value, "unit": "images/sec",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": args.precision, "data": "synthetic", "rccl_ranks": world, "gather": "engine_rccl" if engine_comm else ("torch.distributed" if world > 1 else None),
        "backend": ("gloo (PD_BENCH_REHEARSE: every rank on device 0)" if rehearse else "nccl (RCCL)") if world > 1 else "none (single process)",
        "rank_ms_per_step": {"min": min(rank_ms), "max": max(rank_ms), "per_rank": rank_ms},
        "config": {"workload": f"SD1.5 UNet + Prompt-Diffusion ControlNet, {args.size}x{args.size}, {S}-step DDIM (eta 0), "
                               f"CFG 7.5, bs={B} per GPU (forward batch {2 * B}), random-init weights",
                   "global_batch": world * B, "latent": [h, w], "ddim_steps": S, "parallelism": f"batch-shard x{world}",
                   "stream_f32": bool(args.stream_f32), "controlnet_stream_overlap": not args.single_stream},
    }
    if rank == 0:
        # whole-path MFMA fraction against the algorithmic (hoisted) FLOP count of SURVEY.md §8d -- minus, when the CFG pair's shared
        # front ran once (stat cfg_shared), the contractions that were not executed: "stays in the denominator only if executed"
        gf_fwd = GF_PER_FWD_SAMPLE_64 * (h * w) / 4096.0 if (h, w) != (64, 64) else GF_PER_FWD_SAMPLE_64
        shared = eng.stat("cfg_shared")
        gf_saved_pair = shared_front_gf(h, w, fused_tail=args.precision in ("f16", "bf16") and not args.stream_f32) if shared == 3 else 0.0
        tflop_image_ref = 2 * S * gf_fwd / 1e3
        tflop_image = S * (2 * gf_fwd - gf_saved_pair) / 1e3
        result["path_tflops_per_gpu"] = value / world * tflop_image
        result["cfg_shared_front"] = {
            "on": shared == 3, "stat_cfg_shared": shared,
            "what": "p_sample_ddim feeds cat([x]*2), cat([t]*2) and the same example pair / query to both halves of the CFG batch "
                    "(ddim_hacked.py:189-192): the layers in front of the first cross-attention (conv_in, first ResBlock, first "
                    "SpatialTransformer up to self-attention; UNet and ControlNet) are computed once per pair instead of twice. Exact: "
                    "every layer still runs in every step on every distinct input; option cfg_share / --no-cfg-share turns it off",
            "tflop_per_image_executed": tflop_image, "tflop_per_image_reference_count": tflop_image_ref,
            "path_tflops_per_gpu_at_reference_count": value / world * tflop_image_ref}
        if args.full and shared and world == 1 and not args.no_f32:
            # the same workload with the option off (1 warm-up + 1 timed pass, outside the metric's timed region)
            eng.set_option("cfg_share", 0)
            eng.ddim_sample(**kw)
            torch.cuda.synchronize()
            tq = time.perf_counter()
            o_off = eng.ddim_sample(**kw)
            torch.cuda.synchronize()
            dq = time.perf_counter() - tq
            eng.set_option("cfg_share", 1)
            result["cfg_shared_front"]["value_with_option_off"] = B / dq
            result["cfg_shared_front"]["latents_shared_vs_doubled_max_rel"] = float((out[:B] - o_off).abs().max() / o_off.abs().max())
        if args.full and not args.no_profile:
            # one more pass with HIP events around every contraction launch (not part of the timed region).  It runs
            # single-stream: with ControlNet overlapped on the second stream two kernels share the chip and each one's
            # wall duration no longer measures that kernel alone.
            eng.set_option("two_streams", 0)
            eng.set_option("profile", 1)
            eng.ddim_sample(**kw)
            # f16 MFMA runs at the bf16 rate (MI355X_MICROARCH.md "the F16 forms take the same cycles"); f16x2 issues two
            # fp16 MFMAs per 4 K-elements where f16 issues one per 8: a quarter of the fp16 rate
            peak = {"bf16": PEAK_BF16_TFLOPS, "f16": PEAK_BF16_TFLOPS, "f16x2": PEAK_BF16_TFLOPS / 4, "f32": PEAK_F32_TFLOPS}[args.precision]
            classes = {}
            for name, k in (("igemm_kernel[conv3x3]", 0), ("igemm+rgemm_kernel[linear/conv1x1]", 1), ("conv3x3_patch_kernel", 3),
                            ("attn_kernel", 2), ("st_tail_kernel", 4)):
                ms, n, fl = eng.profile_read(k)
                classes[name] = dict(ms=ms, launches=n, avg_us=1e3 * ms / max(n, 1), tflops=fl / max(ms, 1e-9) / 1e9)
            # HBM view of the short-K linear layers (K <= 1280: the igemm launches that are bandwidth- rather than
            # MFMA-bound): algorithmic bytes = the A rows + the weights + the output, bf16, each moved once
            import csv, tempfile
            with tempfile.NamedTemporaryFile("r", suffix=".csv") as tf:
                eng.profile_dump(tf.name)
                allrows = list(csv.DictReader(open(tf.name)))
            eb = 4 if args.precision in ("f32", "f16x2") else 2

            def alg_bytes(r):   # A rows (a conv3x3 reads its input once, not once per tap) + weights + output, each moved once
                M, N, K = int(r["M"]), int(r["N"]), int(r["K"])
                taps = 9 if int(r["taps"]) >= 90 else 1
                return (M * (K // taps) + N * K + M * N) * eb
            rows = [r for r in allrows if r["klass"] == "1" and int(r["K"]) <= 1280]
            ig = [r for r in allrows if r["klass"] in ("0", "1")]
            alg_per_launch = sum(alg_bytes(r) for r in ig) / max(len(ig), 1)
            if rows:
                by = sum(alg_bytes(r) for r in rows)
                ms_s = sum(float(r["ms"]) for r in rows)
                classes["igemm+rgemm_kernel[linear, K<=1280: HBM view]"] = dict(
                    ms=ms_s, launches=len(rows), avg_us=1e3 * ms_s / len(rows), algorithmic_gb_per_s=by / ms_s / 1e6,
                    frac_of_8_tb_s=by / ms_s / 1e6 / 8000.0)
            # cross-check of the FLOP accounting: what the engine's own per-launch records add up to for this pass (every contraction
            # launch, 2*M*N*K with logical channel counts; the hoisted per-call setup included) against the analytic executed count
            _, n_all, fl_all = eng.profile_read(-1)
            result["cfg_shared_front"]["tflop_per_image_recorded_by_engine"] = fl_all / 1e12 / B
            result["cfg_shared_front"]["contraction_launches_per_pass"] = n_all
            eng.set_option("profile", 0)
            eng.set_option("two_streams", 0 if args.single_stream else 1)
            # dominant kernel family by device time: the generic contraction kernels -- igemm_kernel (every instantiation: linear /
            # conv1x1 / generic conv3x3) and, since round 3, rgemm_kernel (gemm_ring.hip: the short-K linear layers).
            # Each bracket is ONE launch of that kernel (split-K finalize excluded), so avg_launch_us is comparable
            # with rocprofv3's call-weighted average over the igemm_kernel<...> rows (profiles/).
            # (the HBM-view entry above is a sub-population of igemm+rgemm_kernel[linear/conv1x1], not added again)
            ms_g = classes["igemm_kernel[conv3x3]"]["ms"] + classes["igemm+rgemm_kernel[linear/conv1x1]"]["ms"]
            n_g = classes["igemm_kernel[conv3x3]"]["launches"] + classes["igemm+rgemm_kernel[linear/conv1x1]"]["launches"]
            fl_g = sum(classes[k]["tflops"] * classes[k]["ms"] for k in ("igemm_kernel[conv3x3]", "igemm+rgemm_kernel[linear/conv1x1]"))
            achieved = fl_g / max(ms_g, 1e-9)
            # HBM traffic per launch: PMC counters cannot be collected from inside this process; tools/final_measure.sh runs
            # the FETCH_SIZE / WRITE_SIZE passes on this same command line (50-step workload) and commits the summary
            traffic, traffic_source = None, None
            prof_files = sorted(f for f in os.listdir(os.path.join(ROOT, "profiles")) if f.endswith("_pmc_traffic.json"))
            tpath = os.path.join(ROOT, "profiles", prof_files[-1]) if prof_files else ""
            if tpath and os.path.exists(tpath):
                with open(tpath) as f:
                    tj = json.load(f)
                traffic = tj.get("igemm_kernel_hbm_bytes_per_launch")
                traffic_source = "profiles/" + prof_files[-1] + ": " + tj.get("source", "")
            # counter-backed MFMA-pipe utilisation per kernel family (tools/final_measure.sh, same 20-step workload)
            mfma_util, util_source = None, None
            util_files = sorted(f for f in os.listdir(os.path.join(ROOT, "profiles")) if f.endswith("_pmc_mfma_util.json"))
            if util_files:
                with open(os.path.join(ROOT, "profiles", util_files[-1])) as f:
                    uj = json.load(f)
                mfma_util = {k: v.get("mfma_util") for k, v in uj.get("by_kernel", {}).items()}
                util_source = "profiles/" + util_files[-1] + ": " + uj.get("definition", "")
            # trace-derived figures of the same families (tools/roofline_from_trace.py over the kernel trace of this command line)
            trace = None
            rl_files = sorted(f for f in os.listdir(os.path.join(ROOT, "profiles")) if f.endswith("_roofline.json"))
            if rl_files:
                with open(os.path.join(ROOT, "profiles", rl_files[-1])) as f:
                    tj2 = json.load(f)
                fam = tj2.get("families", {}).get("igemm_kernel + rgemm_kernel")
                if fam:
                    trace = {"avg_launch_us": fam["trace_avg_us"], "tflops": fam["tflops"], "frac": fam["frac_of_2500"],
                             "source": "profiles/" + rl_files[-1] + ": " + tj2.get("source", "")}
            ov_us = eng.stat("event_overhead_ns") / 1e3
            result["roofline"] = {"bound": "mfma", "kernel": "igemm_kernel + rgemm_kernel (implicit-GEMM conv / linear: every instantiation of gemm.hip and gemm_ring.hip)",
                                  "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
                                  "traffic": traffic, "traffic_source": traffic_source,
                                  "mfma_util": mfma_util, "mfma_util_source": util_source,
                                  "algorithmic_bytes_per_launch": alg_per_launch,
                                  "traffic_over_algorithmic": (traffic / alg_per_launch) if traffic else None,
                                  "avg_launch_us": 1e3 * ms_g / max(n_g, 1), "launches": n_g,
                                  "avg_launch_us_raw_bracket": 1e3 * ms_g / max(n_g, 1) + ov_us,
                                  "event_bracket_overhead_us": ov_us,
                                  "event_bracket_calibration": "back-to-back event pairs with nothing between them",
                                  "trace": trace,
                                  "flop_per_launch": 1e9 * fl_g / max(n_g, 1), "device_ms_per_pass": ms_g, "by_kernel": classes}
        if args.full:
            # first-stage decode of the 8 latents, outside the metric's timed region: reported for context
            try:
                eng.vae_decode(out[:B])
                torch.cuda.synchronize()
                tv = time.perf_counter()
                img = eng.vae_decode(out[:B])
                torch.cuda.synchronize()
                result["vae_decode_ms"] = 1e3 * (time.perf_counter() - tv)
                assert torch.isfinite(img).all()
            except Exception as ex:   # noqa: BLE001 - context only
                result["vae_decode_ms"] = f"failed: {ex}"
        if args.full and not args.no_parity and world == 1:
            eng.close()
            result["parity"] = parity_leg(E, W, args.precision, args.stream_f32, local)
        if args.full and not args.no_f32 and world == 1 and args.precision in ("f16", "bf16"):
            # the f16x2 mode (split fp16 operands over fp32 storage: fp32-class results, ~5e-6 per step against every
            # reference fixture) on the same workload: 1 warm-up + 1 timed pass.  The fp32-MFMA mode is `--precision f32`.
            eng.close()
            e2 = E.Engine(cfg, device=local, precision="f16x2")
            e2.init_random_weights(1234)
            e2.ddim_sample(**kw)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            o2 = e2.ddim_sample(**kw)
            torch.cuda.synchronize()
            d2 = time.perf_counter() - t1
            assert torch.isfinite(o2).all()
            result["f16x2_mode"] = {"value": B / d2, "unit": "images/sec", "ms_per_step": 1e3 * d2, "dtype": "f16x2",
                                    "path_tflops": B / d2 * tflop_image}
            e2.close()
        if args.full and not args.no_sd3 and world == 1 and args.precision in ("f16", "bf16"):
            result["sd3_leg"] = sd3_leg(args.precision, local)
        if args.full and not args.no_cpu_baseline and world == 1:
            result["cpu_baseline"] = cpu_baseline(S)
        print(json.dumps(result))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    eng.close()


if __name__ == "__main__":
    main()
