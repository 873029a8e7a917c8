"""NumPy restatement of cv2.Canny(img, low, high) as OpenCV's portable C++ path computes it (canny.cpp, aperture 3, L2gradient = False):
the specification the engine's kernels (csrc/canny.hip) are held to byte for byte.  Integer arithmetic throughout.

  canny_states(img, low, high)  uint8 [H, W] or [H, W, C] -> state map [H, W]: 0 not a candidate, 1 weak, 2 strong
  hysteresis(states)            state map -> state map with every weak pixel 8-connected, through candidates, to a strong one set to 2
  canny(img, low, high)         the edge map: 255 where hysteresis(canny_states(...)) == 2, else 0

plus the seeded test pictures shared by the CPU and the GPU tests."""
import numpy as np

NONE, WEAK, STRONG = 0, 1, 2
TG22 = 13573   # tan(22.5 deg) * 2^15


def sobel(img):
    """int32 (dx, dy) [H, W, C] of a [H, W, C] picture: 3x3 Sobel over replicated borders"""
    p = np.pad(img.astype(np.int32), ((1, 1), (1, 1), (0, 0)), mode="edge")
    H, W = img.shape[:2]
    s = lambda r, c: p[1 + r:1 + r + H, 1 + c:1 + c + W]   # the picture shifted by [row, col]
    dx = (s(-1, 1) + 2 * s(0, 1) + s(1, 1)) - (s(-1, -1) + 2 * s(0, -1) + s(1, -1))
    dy = (s(1, -1) + 2 * s(1, 0) + s(1, 1)) - (s(-1, -1) + 2 * s(-1, 0) + s(-1, 1))
    return dx, dy


def gradients(img):
    """(dx, dy, m) [H, W] after the channel select: the channel with the largest |dx| + |dy|, the lowest index on a tie"""
    img = np.asarray(img)
    if img.dtype != np.uint8:
        raise ValueError("uint8 expected")
    if img.ndim == 2:
        img = img[:, :, None]
    dx, dy = sobel(img)
    n = np.abs(dx) + np.abs(dy)
    k = np.argmax(n, axis=2)[:, :, None]   # argmax returns the first maximum
    pick = lambda a: np.take_along_axis(a, k, axis=2)[:, :, 0]
    return pick(dx), pick(dy), pick(n)


def canny_states(img, low, high):
    lo, hi = int(np.floor(low)), int(np.floor(high))
    if lo > hi:
        lo, hi = hi, lo
    dx, dy, m = gradients(img)
    H, W = m.shape
    mp = np.pad(m, 1)                                        # magnitude 0 outside the picture
    nb = lambda r, c: mp[1 + r:1 + r + H, 1 + c:1 + c + W]   # m[row + r, col + c]
    x = np.abs(dx).astype(np.int64)
    y = np.abs(dy).astype(np.int64) << 15
    t22 = x * TG22
    t67 = t22 + (x << 16)
    horizontal = y < t22
    vertical = ~horizontal & (y > t67)
    diagonal = ~horizontal & ~vertical
    keep_h = (m > nb(0, -1)) & (m >= nb(0, 1))
    keep_v = (m > nb(-1, 0)) & (m >= nb(1, 0))
    keep_pos = (m > nb(-1, -1)) & (m > nb(1, 1))   # s = +1
    keep_neg = (m > nb(-1, 1)) & (m > nb(1, -1))   # s = -1
    s_neg = (dx ^ dy) < 0
    cand = (m > lo) & ((horizontal & keep_h) | (vertical & keep_v) | (diagonal & np.where(s_neg, keep_neg, keep_pos)))
    states = np.zeros((H, W), np.uint8)
    states[cand] = WEAK
    states[cand & (m > hi)] = STRONG
    return states


def hysteresis(states):
    """Plain flood from the strong pixels over 8-connected weak ones (a stack, no library)."""
    st = np.array(states, dtype=np.uint8, copy=True)
    H, W = st.shape
    stack = list(zip(*np.nonzero(st == STRONG)))
    while stack:
        r, c = stack.pop()
        for rr in range(max(r - 1, 0), min(r + 2, H)):
            for cc in range(max(c - 1, 0), min(c + 2, W)):
                if st[rr, cc] == WEAK:
                    st[rr, cc] = STRONG
                    stack.append((rr, cc))
    return st


def canny(img, low, high):
    return np.where(hysteresis(canny_states(img, low, high)) == STRONG, 255, 0).astype(np.uint8)


def canny_batch(imgs, low, high):
    return np.stack([canny(i, low, high) for i in imgs])


# ------------------------------------------------------------------ test pictures
BLOB_SIZES = [(37, 53), (64, 64), (130, 67)]
BLOB_THRESHOLDS = [(100, 200), (200, 100), (50.5, 50.5)]


def blobs(H, W, C, B=3, seed=0):
    """clip(128 + 600 gaussian_filter(N(0, 1), sigma 3 in H and W) + 4 N(0, 1), 0, 255) as uint8 [B, H, W, C]"""
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    f = ndimage.gaussian_filter(rng.standard_normal((B, H, W, C)), (0, 3, 3, 0))
    return np.clip(128 + 600 * f + 4 * rng.standard_normal((B, H, W, C)), 0, 255).astype(np.uint8)


def spiral(N=192, value=30, pitch=12, width=3, block=255):
    """[N, N] grey, background 0: a `width`-pixel square spiral of `value` from the outside in, turns `pitch` apart, and a 12 x 12 block
    of `block` over its outer end"""
    img = np.zeros((N, N), np.uint8)
    x0, y0, x1, y1 = 8, 8, N - 9, N - 9
    pts = []
    while x1 - x0 > 2 * pitch and y1 - y0 > 2 * pitch:
        pts += [(y0, x0), (y0, x1), (y1, x1), (y1, x0 + pitch)]
        x0 += pitch
        y0 += pitch
        x1 -= pitch
        y1 -= pitch
        pts.append((y0, x0))
    for (a, b), (c, d) in zip(pts[:-1], pts[1:]):
        ya, yb = sorted((a, c))
        xa, xb = sorted((b, d))
        img[ya:yb + width, xa:xb + width] = value
    img[4:16, 4:16] = block
    return img


def serpentine(N=200):
    """State map [N, N]: every second row weak, joined alternately at the right and the left end into one path, whose first pixel
    (0, 0) is strong; and a detached weak segment in the last row.  Returns (states, path mask, segment mask)."""
    st = np.zeros((N, N), np.uint8)
    rows = list(range(0, N - 3, 2))
    for i, r in enumerate(rows):
        st[r, :] = WEAK
        if i + 1 < len(rows):
            st[r + 1, N - 1 if i % 2 == 0 else 0] = WEAK
    path = st == WEAK
    st[0, 0] = STRONG
    seg = np.zeros((N, N), bool)
    seg[N - 1, 100:110] = True
    st[seg] = WEAK
    return st, path, seg
