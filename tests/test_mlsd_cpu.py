"""M-LSD line detector, the parts that need no GPU: the NumPy contract of the decode and the rasteriser (tests/mlsd_ref.py) against the
reference's own segment lists (tests/golden/mlsd.npz, made by tests/golden/make_golden_mlsd.py from the reference's pred_lines), the
BatchNorm folding of the loader against an unfused fp64 evaluation, the tensor inventory, and the annotator's argument checks."""
import json
import os

import numpy as np
import pytest

from prompt_diffusion_amd import annotators as A
from prompt_diffusion_amd import weights as W
from tests import mlsd_ref as R


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "mlsd.npz"))


def canon(segs):
    segs = np.asarray(segs, np.int32).reshape(-1, 4)
    return segs[np.lexsort(segs.T[::-1])]


# ------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("tag,b", [("tiny", 0), ("tiny", 1), ("sq", 0), ("hand", 0), ("hand", 1)])
def test_decode_matches_the_reference_segments(fx, tag, b):
    thr_v, thr_d = fx["hand_thr"] if tag == "hand" else fx["thr"]
    got = R.decode(fx[tag + "_tp"][b], thr_v, thr_d)
    want = fx[f"{tag}_segs_{b}"]
    assert 20 <= len(want) <= 200
    assert np.array_equal(canon(got), canon(want))


def test_decode_keeps_at_most_200_and_ranks_by_score(fx):
    tp = fx["hand_tp"][1]                      # 230 peaks
    every = R.decode(tp, 0.0, -1.0)            # nothing filtered: exactly the 200 best
    assert len(every) == R.TOPK
    first = every[0]
    y, x = np.unravel_index(np.argmax(tp[0]), tp[0].shape)
    assert first[0] == int(2.0 * (x + np.float64(tp[1, y, x]))) and first[1] == int(2.0 * (y + np.float64(tp[2, y, x])))


def test_decode_of_a_map_without_survivors_is_empty(fx):
    tp = fx["hand_tp"][0]
    assert R.decode(tp, 0.9999, 5.0).shape == (0, 4)
    assert R.decode(tp, 0.05, 1e6).shape == (0, 4)
    assert not R.draw_segments(R.decode(tp, 0.9999, 5.0), 96, 96).any()


# ------------------------------------------------------------------------------------------------ rasteriser
def test_raster_axis_aligned_and_diagonal_lines():
    img = R.draw_segments([[2, 5, 20, 5]], 16, 24)
    assert img[5, 2:21].all() and img.sum() == 19 * 255
    assert np.array_equal(img, R.draw_segments([[20, 5, 2, 5]], 16, 24))
    img = R.draw_segments([[7, 1, 7, 14]], 16, 24)
    assert img[1:15, 7].all() and img.sum() == 14 * 255
    assert np.array_equal(img, R.draw_segments([[7, 14, 7, 1]], 16, 24))
    img = R.draw_segments([[1, 1, 12, 12]], 16, 24)
    assert all(img[i, i] for i in range(1, 13)) and img.sum() == 12 * 255
    img = R.draw_segments([[12, 1, 1, 12]], 16, 24)
    assert all(img[13 - i, i] for i in range(1, 13)) and img.sum() == 12 * 255
    img = R.draw_segments([[5, 5, 5, 5]], 16, 24)
    assert img[5, 5] == 255 and img.sum() == 255


@pytest.mark.parametrize("H,W,seg", R.RASTER_CASES)
def test_raster_case_properties(H, W, seg):
    """What every 8-connected line of thickness 1 has: one pixel per step of the longer axis, every step to a neighbour, both (clipped)
    ends set; a segment that misses the image leaves it blank."""
    img = R.draw_segments([seg], H, W)
    x0, y0, x1, y1 = seg
    inside = lambda x, y: 0 <= x < W and 0 <= y < H
    ys, xs = np.nonzero(img)
    if inside(x0, y0) and inside(x1, y1):
        assert len(ys) == max(abs(x1 - x0), abs(y1 - y0)) + 1
        assert img[y0, x0] == 255 and img[y1, x1] == 255
    ok, cx0, cy0, cx1, cy1 = R.clip_line(W, H, x0, y0, x1, y1)
    if not ok:
        assert len(ys) == 0
        return
    assert inside(cx0, cy0) and inside(cx1, cy1)
    assert len(ys) == max(abs(cx1 - cx0), abs(cy1 - cy0)) + 1
    assert img[cy0, cx0] == 255 and img[cy1, cx1] == 255
    order = np.argsort(xs if abs(cx1 - cx0) >= abs(cy1 - cy0) else ys, kind="stable")
    assert np.all(np.abs(np.diff(xs[order])) <= 1) and np.all(np.abs(np.diff(ys[order])) <= 1)


@pytest.mark.parametrize("H,W,seg", R.RASTER_CASES)
def test_raster_matches_cv2(H, W, seg):
    cv2 = pytest.importorskip("cv2")
    img = np.zeros((H, W, 3), np.uint8)
    cv2.line(img, (seg[0], seg[1]), (seg[2], seg[3]), [255, 255, 255], 1)
    assert np.array_equal(img[:, :, 0], R.draw_segments([seg], H, W))


def test_fixture_segments_draw_inside_the_image(fx):
    for tag, b, (H, Wd) in (("tiny", 0, (64, 96)), ("tiny", 1, (64, 96)), ("sq", 0, (128, 128))):
        img = R.draw_segments(fx[f"{tag}_segs_{b}"], H, Wd)
        assert img.shape == (H, Wd) and 0 < (img == 255).sum() < H * Wd and set(np.unique(img)) <= {0, 255}


# ------------------------------------------------------------------------------------------------ folding, names
def test_spec_is_the_reference_inventory(fx):
    inv = [("mlsd." + k, tuple(s)) for k, s in json.loads(str(fx["spec"]))]
    assert inv == [(n, tuple(s)) for n, s, _ in W.mlsd_spec()]
    sd = W.synth_mlsd_state_dict(int(fx["seed"]))
    assert list(sd) == [n for n, _, _ in W.mlsd_spec()]
    assert all(sd[n].shape == tuple(s) for n, s, _ in W.mlsd_spec())
    n_params = sum(int(np.prod(s)) for _, s, k in W.mlsd_spec() if k != "bn_count")
    assert 1.5e6 < n_params < 1.6e6


def test_engine_spec_is_one_weight_and_one_bias_per_conv():
    es = W.mlsd_engine_spec()
    layers = W.mlsd_layers()
    assert len(es) == 2 * len(layers) and len({n for n, _ in es}) == len(es)
    known = {n for n, _, _ in W.mlsd_spec()}
    assert all(n in known for n, _ in es)                       # every engine tensor carries a checkpoint key
    assert es[0] == ("mlsd.backbone.features.0.0.weight", (32, 4, 3, 3)) and es[1] == ("mlsd.backbone.features.0.1.bias", (32,))
    assert es[-2] == ("mlsd.block23.conv3.weight", (16, 64, 1, 1)) and es[-1] == ("mlsd.block23.conv3.bias", (16,))
    dw = sorted({L["cout"] for L in layers if L["groups"] > 1})
    assert dw == [32, 96, 144, 192, 384, 576]
    # the order of the checkpoint is kept
    order = {n: i for i, (n, _, _) in enumerate(W.mlsd_spec())}
    idx = [order[n] for n, _ in es]
    assert idx == sorted(idx)


def test_synthetic_batchnorm_statistics_are_non_trivial():
    sd = W.synth_mlsd_state_dict()
    for n, _, k in W.mlsd_spec():
        if k == "bn_gamma":
            assert abs(float(sd[n].mean()) - 1.0) > 0.1
        elif k == "bn_beta":
            assert abs(float(sd[n].mean())) > 0.02 and float(sd[n].std()) > 0.1
        elif k == "bn_mean":
            assert float(sd[n].std()) > 0.1
        elif k == "bn_var":
            assert float(sd[n].min()) >= 0.5 and abs(float(sd[n].mean()) - 1.0) > 0.1


def test_folding_equals_the_unfused_fp64_evaluation():
    """conv -> BatchNorm(eval) in fp64 against conv with the folded tensors, for a pointwise, a depthwise and a biased conv."""
    sd = W.synth_mlsd_state_dict()
    folded = W.fold_mlsd_state_dict(sd)
    assert list(folded) == [n for n, _ in W.mlsd_engine_spec()]
    assert all(v.dtype == np.float32 for v in folded.values())
    rng = np.random.default_rng(0)
    picks = [L for L in W.mlsd_layers() if L["conv"] in ("backbone.features.2.conv.0.0.", "backbone.features.2.conv.1.0.", "block16.conv1.0.",
                                                         "block23.conv3.")]
    assert len(picks) == 4
    for L in picks:
        p = W.MLSD_PREFIX
        w = sd[p + L["conv"] + "weight"].astype(np.float64)
        cin_g = w.shape[1]
        x = rng.standard_normal((cin_g, 5, 5))                      # one group's input is enough: the fold is per output channel
        centre = lambda wt: np.einsum("ockl,ckl->o", wt, x[:, 1:1 + wt.shape[2], 1:1 + wt.shape[3]])
        y = centre(w) + (sd[p + L["conv"] + "bias"].astype(np.float64) if L["bias"] else 0.0)
        if L["bn"]:
            g, b, m, v = (sd[p + L["bn"] + k].astype(np.float64) for k in ("weight", "bias", "running_mean", "running_var"))
            y = (y - m) / np.sqrt(v + 1e-5) * g + b
        bias_key = p + (L["bn"] or L["conv"]) + "bias"
        wf = folded[p + L["conv"] + "weight"].astype(np.float64)
        got = centre(wf) + folded[bias_key].astype(np.float64)
        scale = np.abs(wf).reshape(wf.shape[0], -1).sum(1) * np.abs(x).max() + np.abs(y)   # one float32 rounding per folded value
        assert np.all(np.abs(got - y) <= 4 * 2.0 ** -24 * scale + 1e-12), L["conv"]


def test_folding_accepts_bare_keys_and_refuses_strangers():
    sd = W.synth_mlsd_state_dict()
    bare = {k[len(W.MLSD_PREFIX):]: v for k, v in sd.items()}
    a, b = W.fold_mlsd_state_dict(sd), W.fold_mlsd_state_dict(bare)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    no_count = {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    assert all(np.array_equal(a[k], v) for k, v in W.fold_mlsd_state_dict(no_count).items())
    with pytest.raises(ValueError, match="not an M-LSD tensor"):
        W.fold_mlsd_state_dict({**sd, "mlsd.block24.weight": np.zeros(1, np.float32)})
    with pytest.raises(KeyError):
        W.fold_mlsd_state_dict({k: v for k, v in sd.items() if k != "mlsd.block15.conv1.1.running_var"})


def test_detector_argument_checks():
    det = A.MLSDdetector(engine=None)
    with pytest.raises(ValueError):
        det(np.zeros((64, 64), np.uint8), 0.1, 0.1)                 # HW: the reference asserts ndim == 3
    with pytest.raises(ValueError):
        det(np.zeros((64, 64, 4), np.uint8), 0.1, 0.1)
    with pytest.raises(ValueError):
        det(np.zeros((64, 64, 3), np.float32), 0.1, 0.1)
    with pytest.raises(ValueError):
        det.detect(np.zeros((64, 64, 3), np.uint8), 0.1, 0.1)       # the batched form wants [B, H, W, 3]
    import prompt_diffusion_amd as P
    assert P.MLSDdetector is A.MLSDdetector
