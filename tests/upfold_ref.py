"""NumPy statement of the upsample-conv fold (csrc/conv_upfold.hip): conv3x3(nearest_x2(x)) as four 2x2-tap phase convolutions over x.

Output pixel (2y + py, 2x + px) sees source rows {y - 1, y} (py = 0) or {y, y + 1} (py = 1), columns alike; its nine taps collapse
into four whose weights are sums of the original ones over S(parity, tap)."""
import numpy as np

S = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}


def repeat2(x):
    return np.repeat(np.repeat(x, 2, axis=2), 2, axis=3)


def fold_weights(w):
    """w [Cout, Cin, 3, 3] -> [4 (phase = 2 py + px), Cout, Cin, 2 (ty), 2 (tx)], summed in w's dtype"""
    out = np.zeros((4,) + w.shape[:2] + (2, 2), w.dtype)
    for py in range(2):
        for px in range(2):
            for ty in range(2):
                for tx in range(2):
                    for ky in S[py, ty]:
                        for kx in S[px, tx]:
                            out[2 * py + px, :, :, ty, tx] += w[:, :, ky, kx]
    return out


def conv3x3_same(x, w, b=None):
    """zero-padded 3x3 cross-correlation, x [B, Cin, H, W], in x's dtype"""
    B, _, H, W = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    y = np.zeros((B, w.shape[0], H, W), np.result_type(x, w))
    for ky in range(3):
        for kx in range(3):
            y += np.einsum("bchw,oc->bohw", xp[:, :, ky:ky + H, kx:kx + W], w[:, :, ky, kx])
    return y if b is None else y + b[None, :, None, None]


def phase_convs(x, wf, b=None):
    """the four phase convs: x [B, Cin, H, W], wf = fold_weights(w) -> [B, Cout, 2H, 2W].  Tap (ty, tx) of phase (py, px) reads
    source pixel (y - 1 + py + ty, x - 1 + px + tx): where the plain 3x3 tap (py + ty, px + tx) reads."""
    B, _, H, W = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    y = np.zeros((B, wf.shape[1], 2 * H, 2 * W), np.result_type(x, wf))
    for py in range(2):
        for px in range(2):
            acc = np.zeros((B, wf.shape[1], H, W), y.dtype)
            for ty in range(2):
                for tx in range(2):
                    acc += np.einsum("bchw,oc->bohw", xp[:, :, py + ty:py + ty + H, px + tx:px + tx + W], wf[2 * py + px, :, :, ty, tx])
            y[:, :, py::2, px::2] = acc
    return y if b is None else y + b[None, :, None, None]
