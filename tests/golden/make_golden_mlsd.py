#!/usr/bin/env python3
"""Generate tests/golden/mlsd.npz (M-LSD line detector) from the REFERENCE itself.

Runs the reference's unmodified ``MobileV2_MLSD_Large`` (annotator/mlsd/models/mbv2_mlsd_large.py) and ``pred_lines``
(annotator/mlsd/utils.py), each loaded from its own file, on the CPU.  ``cv2`` is a stub module whose ``resize`` returns its input
(``pred_lines`` is called with input_shape = the image's own shape, as ``MLSDdetector.__call__`` does, where INTER_AREA is the
identity) and ``Tensor.cuda`` is the identity for the duration of the call.  The weights are the seeded recipe of
prompt-diffusion_amd/weights.py (``synth_mlsd_state_dict``), loaded through ``load_state_dict(strict=True)``.  Only data is stored.

Cases (keys prefixed by the tag), uint8 images from one Philox stream per case:
  tiny   B 2, 64x96:   images, tp [B,9,32,48], segs_<b> int32 [n,4] = [int(v) for v in line] of pred_lines(thr_v, thr_d)
  sq     B 1, 128x128: images, tp [B,9,64,64], segs_0
  hand   a hand-made tp map [2,9,48,48] for the decode op: image 0 has exactly 200 peaks, image 1 has 230; both have a peak in every
         corner and on every border, and a plateau of two equal neighbours.  hand_segs_<b>: the reference's decode of it
  spec   JSON [name, shape] inventory of MobileV2_MLSD_Large.state_dict()

The script asserts that the fixture can see errors (liveliness) and that the reference's selection has margin, so that an engine
whose tp map differs by float32 rounding reproduces the same segments (see check_margins).

Printed summary of the committed fixture (seed 1234):
  [golden] mlsd: 1552624 parameters in 362 tensors
  [golden] mlsd tiny[0]: centre logit +0.06 +- 1.41, 98.9 % of sigmoids in (0.02, 0.98), displacement std 8.2 px, 170 peaks, 89 segments at (0.5, 7.5), min neighbour gap 8.10e-04
  [golden] mlsd tiny[1]: centre logit +0.01 +- 1.41, 99.1 % of sigmoids in (0.02, 0.98), displacement std 8.2 px, 158 peaks, 88 segments at (0.5, 7.5), min neighbour gap 5.52e-04
  [golden] mlsd sq[0]: centre logit -0.22 +- 1.42, 98.9 % of sigmoids in (0.02, 0.98), displacement std 8.7 px, 446 peaks, 149 segments at (0.5, 7.5), min neighbour gap 7.17e-03
  [golden] mlsd hand[0]: 200 peaks, 184 segments at (0.05, 5.0), min neighbour gap 1.81e+01
  [golden] mlsd hand[1]: 230 peaks, 181 segments at (0.05, 5.0), min neighbour gap 1.85e+01
  [golden] wrote tests/golden/mlsd.npz: 477754 bytes

Usage: python tests/golden/make_golden_mlsd.py --reference DIR
"""
import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

CASES = (("tiny", 2, 64, 96, 10), ("sq", 1, 128, 128, 51))   # tag, B, H, W, Philox key (the first keys whose margins hold)
THR_V, THR_D = 0.5, 7.5              # of the network cases
HAND_THR_V, HAND_THR_D = 0.05, 5.0    # of the hand-made map
SEED = 1234
HAND_KEY = 103                       # Philox key of the hand-made map


def images_from_key(key, shape):
    return np.random.Generator(np.random.Philox(key=[83, int(key)])).integers(0, 256, shape, dtype=np.uint8)


def canon(segs):
    """Rows in lexicographic order: the segment SET (torch.topk leaves the order of equal scores open)."""
    segs = np.asarray(segs, np.int32).reshape(-1, 4)
    return segs[np.lexsort(segs.T[::-1])]


def load_file(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def install_stubs():
    cv2 = types.ModuleType("cv2")
    cv2.INTER_AREA = 3
    cv2.resize = lambda img, size, interpolation=None: img   # same size in and out: INTER_AREA is the identity
    sys.modules.setdefault("cv2", cv2)


def reference_decode(utils, tp, thr_v, thr_d):
    """pred_lines' own decode on a given tp map [1, 9, h, w]: the model is a function that returns it."""
    h, w = tp.shape[2] * 2, tp.shape[3] * 2
    img = np.zeros((h, w, 3), np.uint8)
    try:
        lines = utils.pred_lines(img, lambda x: torch.from_numpy(tp), [h, w], thr_v, thr_d)
    except IndexError:          # no survivor: `lines[:, 0]` of an empty array (MLSDdetector's `except: pass`)
        return np.zeros((0, 4), np.int32), np.zeros((0, 4), np.float64)
    return np.array([[int(v) for v in ln] for ln in lines], np.int32).reshape(-1, 4), np.asarray(lines, np.float64)


def check_margins(tag, tp, thr_v, thr_d, lines):
    """The conditions under which float32 rounding differences of the tp map cannot change the selection."""
    c = torch.from_numpy(tp[0, 0])
    heat = torch.sigmoid(c)
    h, w = c.shape
    hmax = torch.nn.functional.max_pool2d(heat[None, None], 3, stride=1, padding=1)[0, 0]
    peaks = torch.nonzero(hmax == heat)
    scores = heat[peaks[:, 0], peaks[:, 1]].numpy()
    order = np.argsort(-scores, kind="stable")
    top = scores[order][:200]
    assert np.abs(top - thr_v).min() > 1e-3, (tag, "score at thr_v")
    assert len(scores) < 200 or scores[order][199] - (scores[order][200] if len(scores) > 200 else 0.0) >= 1e-3, (tag, "200th / 201st")
    disp = tp[0, 1:5]
    dist = np.sqrt((disp[0] - disp[2]) ** 2 + (disp[1] - disp[3]) ** 2)
    pk = peaks.numpy()[order][:200]
    assert np.abs(dist[pk[:, 0], pk[:, 1]] - thr_d).min() > 1e-2, (tag, "dist at thr_d")
    pad = np.full((h + 2, w + 2), -np.inf, np.float32)
    pad[1:-1, 1:-1] = tp[0, 0]
    gap = np.inf
    for y, x in pk:
        win = pad[y:y + 3, x:x + 3].copy()
        d = np.abs(win - win[1, 1])
        d[1, 1] = np.inf
        d[d == 0] = np.inf        # an exact tie is a plateau: both sides keep both pixels
        gap = min(gap, float(d.min()))
    assert gap >= 1e-4, (tag, "neighbour within 1e-4 of a peak", gap)
    if len(lines):
        frac = np.abs(lines - np.round(lines))
        assert frac.min() > 1e-3, (tag, "end point within 1e-3 of an integer")
    return len(scores), gap


def hand_made(rng):
    """[2, 9, 48, 48]: peaks on the cells (3i, 3j) plus the last row / column, strictly decreasing background elsewhere."""
    h = w = 48
    out = np.zeros((2, 9, h, w), np.float32)
    for b, n_peaks in enumerate((200, 230)):
        c = (-20.0 - 0.01 * np.arange(h * w, dtype=np.float64)).reshape(h, w)
        cells = [(3 * i, 3 * j) for i in range(16) for j in range(16)]
        must = [(0, 0), (0, 45), (45, 0), (0, 21), (21, 0)]
        extra = [(47, 47), (47, 10), (10, 47), (47, 22), (22, 47), (47, 0), (0, 47)]     # last row / column, the other corners
        rest = [p for p in cells if p not in must]
        rng.shuffle(rest)
        plateau = (24, 24)                                                             # (24, 24) and (24, 25) share one logit
        rest.remove(plateau)
        chosen = must + extra + [plateau] + rest[:n_peaks - len(must) - len(extra) - 2]
        logits = np.linspace(2.5, -2.5, len(chosen) + 1)
        rng.shuffle(logits)
        for (y, x), v in zip(chosen, logits):
            c[y, x] = v
        c[24, 25] = c[24, 24]
        assert len(chosen) + 1 == n_peaks
        out[b, 0] = c.astype(np.float32)
        # displacements whose doubled end points stay clear of the integers: (k + U(0.05, 0.95)) / 2
        out[b, 1:5] = ((np.floor(rng.uniform(-28.0, 28.0, (4, h, w))) + rng.uniform(0.05, 0.95, (4, h, w))) / 2.0).astype(np.float32)
        out[b, 5:] = rng.standard_normal((4, h, w)).astype(np.float32)
    return out


def run_case(net, utils, mlsd_ref, tag, B, H, Wd, key):
    """One network case: the reference's tp maps and segment lists, with the liveliness and margin assertions."""
    res = {}
    imgs = images_from_key(key, (B, H, Wd, 3))
    tps = []
    for b in range(B):
        caught = {}

        def model(x, caught=caught):
            with torch.no_grad():
                caught["tp"] = net(x)
            return caught["tp"]
        lines = utils.pred_lines(imgs[b], model, [H, Wd], THR_V, THR_D)
        tp = caught["tp"].numpy()
        assert tp.shape == (1, 9, H // 2, Wd // 2)
        segs = np.array([[int(v) for v in ln] for ln in lines], np.int32).reshape(-1, 4)
        # liveliness: the fixture must be able to see an error
        centre, heat, disp = tp[0, 0], 1.0 / (1.0 + np.exp(-tp[0, 0].astype(np.float64))), tp[0, 1:5]
        inside = float(((heat > 0.02) & (heat < 0.98)).mean())
        assert centre.std() >= 1.0, (tag, b, "centre-logit std", float(centre.std()))
        assert inside >= 0.95, (tag, b, "sigmoid inside (0.02, 0.98)", inside)
        assert 2.0 * disp.std() >= 5.0, (tag, b, "displacement std in pixels", 2.0 * float(disp.std()))
        assert 20 <= len(segs) <= 150, (tag, b, "segments", len(segs))
        npeaks, gap = check_margins(f"{tag}[{b}]", tp, THR_V, THR_D, np.asarray(lines, np.float64))
        assert np.array_equal(canon(mlsd_ref.decode(tp[0], THR_V, THR_D)), canon(segs)), (tag, b, "tests/mlsd_ref.py disagrees with pred_lines")
        print(f"[golden] mlsd {tag}[{b}]: centre logit {centre.mean():+.2f} +- {centre.std():.2f}, {100 * inside:.1f} % of sigmoids in (0.02, 0.98), "
              f"displacement std {2.0 * disp.std():.1f} px, {npeaks} peaks, {len(segs)} segments at ({THR_V}, {THR_D}), min neighbour gap {gap:.2e}")
        tps.append(tp[0])
        res[f"{tag}_segs_{b}"] = segs
    res[tag + "_images"] = imgs
    res[tag + "_tp"] = np.stack(tps)
    return res


def run_hand(utils, mlsd_ref, key):
    res = {}
    hand = hand_made(np.random.Generator(np.random.Philox(key=[83, int(key)])))
    for b in range(2):
        segs, lines = reference_decode(utils, hand[b:b + 1], HAND_THR_V, HAND_THR_D)
        npeaks, gap = check_margins(f"hand[{b}]", hand[b:b + 1], HAND_THR_V, HAND_THR_D, lines)
        assert npeaks == (200, 230)[b], (b, npeaks)
        assert np.array_equal(canon(mlsd_ref.decode(hand[b], HAND_THR_V, HAND_THR_D)), canon(segs)), (b, "tests/mlsd_ref.py disagrees with pred_lines")
        print(f"[golden] mlsd hand[{b}]: {npeaks} peaks, {len(segs)} segments at ({HAND_THR_V}, {HAND_THR_D}), min neighbour gap {gap:.2e}")
        res[f"hand_segs_{b}"] = segs
    res["hand_tp"] = hand
    return res


def load_reference(ref):
    install_stubs()
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from prompt_diffusion_amd import weights as W
    import mlsd_ref
    model_mod = load_file("ref_mbv2_mlsd_large", os.path.join(ref, "annotator", "mlsd", "models", "mbv2_mlsd_large.py"))
    utils = load_file("ref_mlsd_utils", os.path.join(ref, "annotator", "mlsd", "utils.py"))
    torch.set_num_threads(8)
    torch.Tensor.cuda = lambda self, *a, **k: self     # pred_lines moves its input to the GPU; there is none here
    sd = W.synth_mlsd_state_dict(SEED)
    net = model_mod.MobileV2_MLSD_Large().eval()
    net.load_state_dict({k[len(W.MLSD_PREFIX):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return W, mlsd_ref, utils, net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, metavar="DIR", help="checkout of the reference project")
    args = ap.parse_args()
    W, mlsd_ref, utils, net = load_reference(os.path.abspath(args.reference))
    inv = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert [("mlsd." + k, tuple(s)) for k, s in inv] == [(n, tuple(s)) for n, s, _ in W.mlsd_spec()], "M-LSD inventory mismatch"
    print(f"[golden] mlsd: {sum(int(np.prod(s)) for _, s in inv if s)} parameters in {len(inv)} tensors")

    res = {"spec": np.array(json.dumps(inv)), "seed": np.array(SEED, np.int64), "thr": np.array([THR_V, THR_D], np.float64),
           "hand_thr": np.array([HAND_THR_V, HAND_THR_D], np.float64)}
    for tag, B, H, Wd, key in CASES:
        res.update(run_case(net, utils, mlsd_ref, tag, B, H, Wd, key))
    res.update(run_hand(utils, mlsd_ref, HAND_KEY))
    out = os.path.join(HERE, "mlsd.npz")
    np.savez_compressed(out, **res)
    print(f"[golden] wrote {out}: {os.path.getsize(out)} bytes")
    assert os.path.getsize(out) < 1000000


if __name__ == "__main__":
    main()
