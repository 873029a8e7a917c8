"""Which kernel family / tile / split every contraction launch of one denoising step takes (engine option verbose = 2, stderr):
python tools/dispatch_trace.py [--batch 8] [--size 512] [--precision f16|bf16|f32|f16x2];  prints the distinct lines with their counts.
--hed traces the 13 trunk convs of the HED edge detector (Engine.hed on a batch of size x size images) instead.
--mlsd traces the 45 contraction launches of the M-LSD line detector (Engine.mlsd) instead, in network order.
--sd3 traces one guided Euler step of the SD3-medium MMDiT + ControlNet (random weights, size x size pixels, 333 context tokens) instead.
PDENGINE_LIB=/path/to/libpdengine.so traces another build of the library (engine.load_library): diff the two outputs to compare builds."""
import argparse, collections, os, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if len(sys.argv) > 1 and sys.argv[1] == "--child":
    from prompt_diffusion_amd import engine as E, weights as W
    B = int(sys.argv[2]); L = int(sys.argv[3]) // 8
    e = E.Engine(W.SD15, precision=sys.argv[4])
    e.init_random_weights(3)
    inp = W.synth_inputs(W.SD15, B, L, L)
    kw = dict(x_T=inp["x_T"], ctx_cond=inp["ctx_cond"], ctx_uncond=inp["ctx_uncond"], pair=inp["pair"], query=inp["query"], steps=50, cfg_scale=7.5)
    e.sample_begin(**kw)
    e.sample_step(0)
    e.set_option("verbose", 2)
    e.sample_step(1)
    e.set_option("verbose", 0)
    e.sample_end()
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "--child-hed":
    import dataclasses
    import numpy as np
    from prompt_diffusion_amd import engine as E, weights as W
    B = int(sys.argv[2]); L = int(sys.argv[3])
    e = E.Engine(dataclasses.replace(W.TINY, hed=True), precision=sys.argv[4])
    e.load_hed_state_dict(W.synth_hed_state_dict())
    x = np.random.default_rng(0).uniform(0, 1, (B, 3, L, L)).astype(np.float32)
    e.hed(x)
    e.set_option("verbose", 2)
    e.hed(x)
    e.set_option("verbose", 0)
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "--child-mlsd":
    import dataclasses
    import numpy as np
    from prompt_diffusion_amd import engine as E, weights as W
    B = int(sys.argv[2]); L = int(sys.argv[3])
    e = E.Engine(dataclasses.replace(W.TINY, mlsd=True), precision=sys.argv[4])
    e.load_mlsd_state_dict(W.synth_mlsd_state_dict())
    x = np.random.default_rng(0).integers(0, 256, (B, L, L, 3), dtype=np.uint8)
    e.mlsd(x, what="tpmap")
    e.set_option("verbose", 2)
    e.mlsd(x, what="tpmap")
    e.set_option("verbose", 0)
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "--child-sd3":
    import torch
    from prompt_diffusion_amd import sd3
    L = int(sys.argv[3]) // 8
    cfg = sd3.SD3Config(pos_embed_max_size=96)
    g = torch.Generator(device="cuda").manual_seed(0)
    f = lambda *s: torch.randn(*s, device="cuda", generator=g)
    x, cond, pair = f(1, 16, L, L), f(1, 16, L, L), f(1, 16, L, L)
    ctx, nctx, pool, npool = f(1, 333, cfg.joint_dim), f(1, 333, cfg.joint_dim), f(1, cfg.pooled_dim), f(1, cfg.pooled_dim)
    e = sd3.SD3Engine(cfg, precision=sys.argv[4])
    e.init_random_weights(7)
    run = lambda: e.sample(x, ctx, pool, nctx, npool, control_latents=cond, pair_latents=pair, num_inference_steps=1, guidance_scale=7.0)
    run()
    e.base.set_option("verbose", 2)
    run()
    e.base.set_option("verbose", 0)
    torch.cuda.synchronize()
    sys.exit(0)
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--precision", default="f16", choices=["f16", "bf16", "f32", "f16x2"])
ap.add_argument("--hed", action="store_true", help="the HED edge detector's trunk instead of a denoising step (launch order kept)")
ap.add_argument("--mlsd", action="store_true", help="the M-LSD line detector's contractions instead (launch order kept)")
ap.add_argument("--sd3", action="store_true", help="one guided Euler step of the SD3-medium MMDiT + ControlNet instead")
a = ap.parse_args()
r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-sd3" if a.sd3 else "--child-mlsd" if a.mlsd else "--child-hed" if a.hed else "--child", str(a.batch), str(a.size), a.precision], capture_output=True, text=True)
if a.hed or a.mlsd:   # in network order
    for l in r.stderr.splitlines():
        if l.startswith("[pdengine] gemm"):
            print(l[len("[pdengine] gemm "):])
    sys.exit(r.returncode)
if r.returncode:
    sys.stderr.write(r.stderr[-2000:])
    sys.exit(r.returncode)
cnt = collections.Counter(l for l in r.stderr.splitlines() if l.startswith("[pdengine] gemm"))
for l, n in sorted(cnt.items(), key=lambda kv: (kv[0].split(":")[1].split()[0], -kv[1])):
    print(f"{n:3d} x {l[len('[pdengine] gemm '):]}")
