"""BASELINE config #4: 768x768, UniPC 20 steps, bs 8, through PromptDiffusionPipeline with the host UniPC plug-in
(random-init SD1.5 weights, synthetic inputs).  Prints images/s; the loop is engine eps evaluations + host scheduler.
--fused: also the same call with fuse_scheduler=True (the UniPC update inside the engine's loop), and both rates.
--scheduler unipc|dpmpp|pndm|ddim: the scheduler (ddim: no plug-in, the engine's own loop on the pipeline's grid);
--only host|fused: one of the two rates alone, for alternating fresh processes."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from prompt_diffusion_amd import engine as E, weights as W
from prompt_diffusion_amd.pipeline import PromptDiffusionPipeline
from prompt_diffusion_amd.schedulers import DPMSolverMultistepScheduler, PNDMScheduler, UniPCMultistepScheduler
fused = "--fused" in sys.argv
argv = [a for a in sys.argv[1:] if a != "--fused"]
opt = {}
for key in ("--scheduler", "--only"):
    if key in argv:
        i = argv.index(key)
        opt[key] = argv[i + 1]
        del argv[i:i + 2]
sname = opt.get("--scheduler", "unipc")
make_sched = {"unipc": UniPCMultistepScheduler, "dpmpp": DPMSolverMultistepScheduler, "pndm": PNDMScheduler, "ddim": lambda: None}[sname]
label = {"unipc": "UniPC", "dpmpp": "DPM-Solver++(2M)", "pndm": "PNDM", "ddim": "DDIM"}[sname]
size = int(argv[0]) if len(argv) > 0 else 768
steps = int(argv[1]) if len(argv) > 1 else 20
B = 8
e = E.Engine(W.SD15, precision="bf16"); e.init_random_weights(1234)
g = np.random.default_rng(0)
pe = g.standard_normal((B, 77, 768), dtype=np.float32); ne = g.standard_normal((B, 77, 768), dtype=np.float32)
img = lambda: g.random((B, size, size, 3), dtype=np.float32)
q, a, b = img(), img(), img()
lat = g.standard_normal((B, 4, size // 8, size // 8), dtype=np.float32)
kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, image=q, image_pair=[a, b], num_inference_steps=steps, guidance_scale=7.5,
          latents=lat, output_type="latent", height=size, width=size)


def rate(fuse):
    pipe = PromptDiffusionPipeline(e, scheduler=make_sched(), fuse_scheduler=fuse and sname != "ddim")
    out = pipe(**kw).images
    t0 = time.perf_counter(); out = pipe(**kw).images; dt = time.perf_counter() - t0
    assert np.isfinite(np.asarray(out)).all()
    name = "engine loop" if sname == "ddim" else "fused" if fuse else "host plug-in"
    print(f"config4 {size}x{size} {label} {steps} steps bs {B} ({name}): {dt*1e3:.1f} ms -> {B/dt:.3f} img/s; "
          f"|lat| mean {np.abs(np.asarray(out)).mean():.4f}")
    return B / dt, np.asarray(out)


if "--only" in opt:
    rate(opt["--only"] == "fused")
    sys.exit(0)
r_host, o_host = rate(False)
if fused:
    r_fused, o_fused = rate(True)
    d = float(np.abs(o_fused - o_host).max() / np.abs(o_host).max())
    print(f"config4 rates: host plug-in {r_host:.3f} img/s, fused {r_fused:.3f} img/s ({r_fused / r_host:.3f}x); "
          f"fused vs host latent relerr {d:.2e}")
