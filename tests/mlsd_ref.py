"""NumPy restatement of the parts of the M-LSD annotator that are not the network: pred_lines' decode
(annotator/mlsd/utils.py:19-86) and cv2.line as MLSDdetector.__call__ uses it (annotator/mlsd/__init__.py:34-36).

This file is the contract of the engine's decode and raster kernels.  The decode is checked against the reference's own segment
lists (tests/golden/mlsd.npz); the rasteriser restates OpenCV's ``clipLine`` + ``LineIterator`` (thickness 1, LINE_8, shift 0) and
is compared with ``cv2.line`` itself only where ``cv2`` imports.

One deliberate difference from the reference, shared with the engine: the 3x3 non-maximum suppression and the ranking run on the
logits, not on their sigmoids.  The sigmoid is monotone, so the two agree wherever float32 sigmoids of different logits differ; the
fixture script asserts that margin.  Among equal logits the lower flat index ranks first.
"""
import numpy as np

TOPK = 200


def decode(tp, thr_v, thr_d, topk=TOPK):
    """tp [9, h, w] float32 -> int32 [n, 4] (x0, y0, x1, y1 in input pixels), best score first: one image of pred_lines with
    input_shape = the image's own shape."""
    tp = np.asarray(tp, np.float32)
    _, h, w = tp.shape
    c = tp[0]
    pad = np.full((h + 2, w + 2), -np.inf, np.float32)
    pad[1:-1, 1:-1] = c
    hmax = np.max(np.stack([pad[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)]), axis=0)
    flat = c.reshape(-1)
    peaks = np.flatnonzero((hmax == c).reshape(-1))
    order = peaks[np.lexsort((peaks, -flat[peaks].astype(np.float64)))][:topk]   # logit descending, then index ascending
    disp = tp[1:5].transpose(1, 2, 0)                                               # [h, w, 4] float32
    start, end = disp[:, :, :2], disp[:, :, 2:]
    dist_map = np.sqrt(np.sum((start - end) ** 2, axis=-1))                         # float32, as utils.py:66
    out = []
    for idx in order:
        y, x = int(idx) // w, int(idx) % w
        score = np.float32(1.0) / (np.float32(1.0) + np.exp(-flat[idx], dtype=np.float32))
        if score > np.float32(thr_v) and dist_map[y, x] > np.float32(thr_d):
            d = disp[y, x]
            seg = 2.0 * np.array([np.int64(x) + d[0], np.int64(y) + d[1], np.int64(x) + d[2], np.int64(y) + d[3]], np.float64)
            out.append([int(v) for v in seg])                                       # int(val): truncation towards zero
    return np.asarray(out, np.int32).reshape(-1, 4)


def clip_line(W, H, x1, y1, x2, y2):
    """cv2.clipLine on Python integers: (inside, x1, y1, x2, y2)."""
    right, bottom = W - 1, H - 1
    code = lambda x, y: (x < 0) + (x > right) * 2 + (y < 0) * 4 + (y > bottom) * 8
    c1, c2 = code(x1, y1), code(x2, y2)
    if (c1 & c2) == 0 and (c1 | c2) != 0:
        if c1 & 12:
            a = 0 if c1 < 8 else bottom
            x1 += int(float(a - y1) * float(x2 - x1) / float(y2 - y1))
            y1 = a
            c1 = (x1 < 0) + (x1 > right) * 2
        if c2 & 12:
            a = 0 if c2 < 8 else bottom
            x2 += int(float(a - y2) * float(x2 - x1) / float(y2 - y1))
            y2 = a
            c2 = (x2 < 0) + (x2 > right) * 2
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                a = 0 if c1 == 1 else right
                y1 += int(float(a - x1) * float(y2 - y1) / float(x2 - x1))
                x1 = a
                c1 = 0
            if c2:
                a = 0 if c2 == 1 else right
                y2 += int(float(a - x2) * float(y2 - y1) / float(x2 - x1))
                x2 = a
                c2 = 0
    return (c1 | c2) == 0, x1, y1, x2, y2


def draw_line(img, p0, p1, value=255):
    """cv2.line(img, p0, p1, value, 1) on a uint8 [H, W] array, in place: clip, then LineIterator(connectivity 8, leftToRight)."""
    H, W = img.shape
    x1, y1, x2, y2 = int(p0[0]), int(p0[1]), int(p1[0]), int(p1[1])
    if not (0 <= x1 < W and 0 <= x2 < W and 0 <= y1 < H and 0 <= y2 < H):
        ok, x1, y1, x2, y2 = clip_line(W, H, x1, y1, x2, y2)
        if not ok:
            return img
    dx, dy = x2 - x1, y2 - y1
    px, py, step_x, step_y = x1, y1, 1, 1
    if dx < 0:
        dx, dy, px, py = -dx, -dy, x2, y2
    if dy < 0:
        dy, step_y = -dy, -1
    vert = dy > dx
    if vert:
        dx, dy = dy, dx
    err, plus, minus = dx - 2 * dy, 2 * dx, -2 * dy
    for _ in range(dx + 1):
        img[py, px] = value
        m = err < 0
        err += minus + (plus if m else 0)
        if vert:
            py += step_y
            px += step_x if m else 0
        else:
            px += step_x
            py += step_y if m else 0
    return img


def draw_segments(segs, H, W):
    """int [n, 4] -> uint8 [H, W] of 0 / 255."""
    img = np.zeros((H, W), np.uint8)
    for s in np.asarray(segs).reshape(-1, 4):
        draw_line(img, (s[0], s[1]), (s[2], s[3]))
    return img


# the rasteriser cases of the CPU and GPU tests: (H, W, [x0, y0, x1, y1])
RASTER_CASES = [
    (16, 24, [2, 5, 20, 5]),        # horizontal
    (16, 24, [20, 5, 2, 5]),        # ... right to left
    (16, 24, [7, 1, 7, 14]),        # vertical
    (16, 24, [7, 14, 7, 1]),
    (16, 24, [1, 1, 12, 12]),       # both diagonals
    (16, 24, [12, 1, 1, 12]),
    (16, 24, [1, 2, 22, 9]),        # shallow, both directions
    (16, 24, [22, 2, 1, 9]),
    (16, 24, [22, 9, 1, 2]),
    (16, 24, [3, 0, 8, 15]),        # steep, both directions
    (16, 24, [8, 0, 3, 15]),
    (16, 24, [3, 15, 8, 0]),
    (16, 24, [5, 5, 5, 5]),         # a single point
    (16, 24, [-9, 3, 10, 11]),      # one end outside each edge
    (16, 24, [10, 3, 40, 12]),
    (16, 24, [4, -7, 15, 9]),
    (16, 24, [4, 9, 15, 30]),
    (16, 24, [-5, -8, 30, 22]),     # both ends outside, crossing
    (16, 24, [-3, 20, 30, -6]),
    (16, 24, [-10, -2, -1, 9]),     # fully outside
    (16, 24, [30, 2, 50, 40]),
    (16, 24, [-4, 18, 40, 25]),
    (16, 24, [0, 0, 23, 15]),       # corner to corner
    (33, 17, [16, 0, 0, 32]),
    (33, 17, [-2, 35, 19, -3]),
]
