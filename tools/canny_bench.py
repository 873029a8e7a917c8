"""The Canny edge detector (Engine.canny): time per call, hysteresis sweeps per call and the split between its three kernels.

    python tools/canny_bench.py [--calls 20]

Workloads, each a batch of uint8 RGB pictures that is already on the device (the uint8 edge map stays there too):
  blobs-512   8 x 512^2 blob pictures (the recipe of tests/canny_ref.py), thresholds 100 / 200
  blobs-768   8 x 768^2 of the same
  spiral-512  8 x 512^2, the faint 192^2 spiral of the tests tiled 3 x 3 and cropped: the long floods that cost sweeps
Per workload one JSON line: the median host-clock time of a synchronised call (which includes the sweeps' flag read-backs), the sweeps
of the last call, the same call from and to host memory, and -- from a separate pass with option "profile" on -- the device time of
the suppression kernel, of all hysteresis sweeps and of the emit kernel per call (pd_profile_read classes 5 / 6 / 7).  Where cv2 is
importable, cv2.Canny's host time for the same batch is printed next to it and its bytes are compared; otherwise the line says that
the comparison is unmeasured.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B = 8


def workloads():
    import numpy as np

    from tests import canny_ref as R
    sp = np.tile(R.spiral(), (3, 3))[:512, :512]
    return {
        "blobs-512": R.blobs(512, 512, 3, B=B, seed=11),
        "blobs-768": R.blobs(768, 768, 3, B=B, seed=12),
        "spiral-512": np.ascontiguousarray(np.broadcast_to(sp[None, :, :, None], (B, 512, 512, 3))),
    }


def timed(fn, calls, sync):
    ts = []
    for _ in range(calls):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch

    from prompt_diffusion_amd import engine as E
    from prompt_diffusion_amd import weights as W
    try:
        import cv2
    except ImportError:
        cv2 = None
    if not torch.cuda.is_available():
        sys.exit("canny_bench needs a GPU")
    e = E.Engine(W.TINY, precision="f32")
    sync = torch.cuda.synchronize
    for name, img in workloads().items():
        dev = torch.from_numpy(img).cuda()
        lo, hi = 100, 200
        got = e.canny(dev, lo, hi)                         # warm-up, and the bytes every later call must repeat
        e.canny(img, lo, hi)
        t_dev = timed(lambda: e.canny(dev, lo, hi), args.calls, sync)
        sweeps = e.stat("canny_sweeps")
        t_host = timed(lambda: e.canny(img, lo, hi), args.calls, sync)
        assert torch.equal(e.canny(dev, lo, hi), got)
        e.set_option("profile", 1)
        for _ in range(args.calls):
            e.canny(dev, lo, hi)
        split = {k: e.profile_read(klass) for k, klass in (("nms", 5), ("hysteresis", 6), ("emit", 7))}
        e.set_option("profile", 0)
        row = dict(leg=name, pictures=B, size=list(img.shape[1:3]), edge_fraction=round(float((got == 255).float().mean()), 4),
                   device_call_ms=round(1e3 * t_dev, 3), sweeps=sweeps, host_call_ms=round(1e3 * t_host, 3),
                   kernel_ms_per_call={k: round(ms / args.calls, 4) for k, (ms, n, _) in split.items()},
                   hysteresis_launches_per_call=split["hysteresis"][1] / args.calls)
        if cv2 is not None:
            ref = np.stack([cv2.Canny(i, lo, hi) for i in img])
            row["cv2_host_ms"] = round(1e3 * timed(lambda: [cv2.Canny(i, lo, hi) for i in img], args.calls, lambda: None), 3)
            row["identical_to_cv2"] = bool(np.array_equal(ref, got.cpu().numpy()))
        else:
            row["cv2_host_ms"] = "unmeasured: cv2 is not installed here"
        print(json.dumps(row), flush=True)
    e.close()


if __name__ == "__main__":
    main()
