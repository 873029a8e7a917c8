"""fp64 NumPy statement of the adapter arithmetic (DESIGN.md §7 "LoRA adapters"), and the error budget of the fp32 merge.

A *term* is a dict: ``kind`` ("pair", "hada", "kron"), ``up`` / ``down`` (and ``up2`` / ``down2`` for "hada"; w1 / w2 for "kron"),
``scale`` (alpha / r; 1 when absent), ``s`` (the adapter's multiplier), and an optional ``magnitude`` [N].  With N rows and
K = cin * kh * kw columns in checkpoint order,

  pair   D = scale * up @ down
  hada   D = scale * (up @ down) * (up2 @ down2)
  kron   D[i c + p, j d + q, y, x] = scale * w1[i, j] * w2[p, q, y, x]
  E = s D                                        without a magnitude
  E = (m / n) (W0 + s D) - W0, n = |W0 + s D|_2 per row (factor 0 where n = 0)    with one
  W = W0 + sum of E over the terms with s != 0

``merge`` returns W and, per element, ``tol32``: a bound on what the fp32 evaluation can differ from W by, before the one rounding
to the storage type.  With eps = 2^-23 (every fp32 operation is within 2^-24 relative; the factor 2 pays for products that are not
fused and for second-order terms):

  * s D is a chain of `ops` operations on terms whose absolute values sum to `mag`: the two scale products, then r fused
    multiply-adds (pair: ops = R + 2 with R the ranks of all plain pairs of the tensor, which share one chain; hada: r1 + r2 + 3 on
    mag = mag1 * mag2; kron: 3).  |fl(s D) - s D| <= ops * eps * mag.
  * Each term is added to a running sum that starts at W0: one rounding of a partial sum, itself at most |W0| + sum of |E|-bounds.
    A magnitude term costs a second one for its own "- W0".
  * Under a magnitude, v = W0 + s D carries the error above plus its own rounding, at most (ops + 1) eps V with V = |W0| + mag.
    The row norm is a sum of K squares (chain and tree: at most K + 1 roundings, halved by the root, plus the root's own), so
    |fl(n) - n| <= eps ((ops + 1) |V|_2 + (K / 2 + 2) n) <= eps (ops + K / 2 + 3) |V|_2.  The factor m / n adds the division, the
    product f v one more, the subtraction one on |f v| + |W0|.  Together
        |fl(E) - E| <= eps |f| V (ops + 5 + (ops + K / 2 + 3) |V|_2 / n) + eps |W0|.
"""
import numpy as np

EPS = 2.0 ** -23


def _f32(x):
    return float(np.float32(x))


def tucker_fold(t, wb):
    """sum_j t[i, j, y, x] wb[j, c] -> [r, cin, kh, kw], in fp64"""
    return np.einsum("ijyx,jc->icyx", np.asarray(t, np.float64), np.asarray(wb, np.float64))


def term(kind, f, alpha, s, shape, magnitude=None):
    """A term from an adapter's own factors (roles as in the key names: up / down / mid; w1_a, w1_b, w2_a, w2_b, t1, t2; w1 or w1_a +
    w1_b, w2 or w2_a + w2_b (+ t2)), folded in fp64.  `extra_ops` counts the roundings of a host fold to fp32 (one per folded factor)."""
    a64 = lambda x: np.asarray(x, np.float64)
    N, cin = int(shape[0]), int(shape[1])
    out = dict(s=s, magnitude=magnitude, extra_ops=0)
    if kind == "lora":
        up, down = a64(f["up"]).reshape(N, -1), a64(f["down"])
        r = down.shape[0]
        if "mid" in f:
            down = tucker_fold(f["mid"], down.reshape(r, cin))
            out["extra_ops"] = 1
        out.update(kind="pair", up=up, down=down)
    elif kind == "loha":
        r = np.asarray(f["w1_b"]).shape[0]
        if "t1" in f:
            out.update(kind="hada", up=a64(f["w1_a"]).T, down=tucker_fold(f["t1"], f["w1_b"]), up2=a64(f["w2_a"]).T,
                       down2=tucker_fold(f["t2"], f["w2_b"]), extra_ops=2)
        else:
            out.update(kind="hada", up=a64(f["w1_a"]), down=a64(f["w1_b"]), up2=a64(f["w2_a"]), down2=a64(f["w2_b"]))
    elif kind == "lokr":
        r = None
        if "w1" in f:
            w1 = a64(f["w1"])
        else:
            w1, r = a64(f["w1_a"]) @ a64(f["w1_b"]), np.asarray(f["w1_b"]).shape[0]
            out["extra_ops"] += 1
        if "w2" in f:
            w2 = a64(f["w2"])
        elif "t2" in f:
            w2, r = np.einsum("ijyx,ip,jq->pqyx", a64(f["t2"]), a64(f["w2_a"]), a64(f["w2_b"])), np.asarray(f["t2"]).shape[0]
            out["extra_ops"] += 1
        else:
            w2, r = a64(f["w2_a"]) @ a64(f["w2_b"]), np.asarray(f["w2_b"]).shape[0]
            out["extra_ops"] += 1
        w2 = w2.reshape(N // w1.shape[0], cin // w1.shape[1], -1)
        out.update(kind="kron", up=w1, down=w2)
        if r is None:
            alpha = None
    else:
        raise ValueError(kind)
    out["scale"] = 1.0 if alpha is None else float(alpha) / r
    return out


def scaled_delta(term, shape):
    """(s D, mag, ops) of one term as fp64 [N, K]; ops without the shared plain chain (see merge)"""
    N, K = int(shape[0]), int(np.prod(shape[1:]))
    c = _f32(term["s"]) * _f32(term.get("scale", 1.0))
    a64 = lambda x: np.asarray(x, np.float64)
    kind = term["kind"]
    if kind in ("pair", "hada"):
        u, d = a64(term["up"]).reshape(N, -1), a64(term["down"])
        d = d.reshape(d.shape[0], K)
        D, mag, ops = c * (u @ d), abs(c) * (np.abs(u) @ np.abs(d)), u.shape[1] + 2
        if kind == "hada":
            u2, d2 = a64(term["up2"]).reshape(N, -1), a64(term["down2"])
            d2 = d2.reshape(d2.shape[0], K)
            D, mag, ops = D * (u2 @ d2), mag * (np.abs(u2) @ np.abs(d2)), ops + u2.shape[1] + 1
        return D, mag, ops + term.get("extra_ops", 0)
    if kind == "kron":
        w1, w2 = a64(term["up"]), a64(term["down"])
        w2 = w2.reshape(w2.shape[0], w2.shape[1], -1)
        D = c * np.einsum("ij,pqt->ipjqt", w1, w2).reshape(N, K)
        return D, np.abs(D), 3 + term.get("extra_ops", 0)
    raise ValueError(kind)


def merge(w0, terms):
    """(W, tol32) in fp64, shaped like w0 (the base weights as the engine stores them)"""
    shape = w0.shape
    N, K = int(shape[0]), int(np.prod(shape[1:]))
    w0 = np.asarray(w0, np.float64).reshape(N, K)
    active = [t for t in terms if _f32(t["s"]) != 0.0]
    r_plain = sum(np.asarray(t["up"]).reshape(N, -1).shape[1] for t in active if t["kind"] == "pair" and t.get("magnitude") is None)
    W = w0.copy()
    err = np.zeros_like(w0)       # sum of ops * mag
    reach = np.abs(w0)            # bound of every partial sum
    adds = 0
    for t in active:
        D, mag, ops = scaled_delta(t, shape)
        m = t.get("magnitude")
        if m is None:
            if t["kind"] == "pair":
                ops = r_plain + 2
            W += D
            err += ops * mag
            reach += mag
            adds += 1
            continue
        m = np.asarray(m, np.float64).reshape(N, 1)
        v = w0 + D
        V = np.abs(w0) + mag
        n = np.sqrt((v * v).sum(axis=1, keepdims=True))
        Vn = np.sqrt((V * V).sum(axis=1, keepdims=True))
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.where(n > 0, m / n, 0.0)
            ratio = np.where(n > 0, Vn / n, 0.0)
        W += f * v - w0
        err += np.abs(f) * V * (ops + 5 + (ops + K / 2 + 3) * ratio) + np.abs(w0)
        reach += np.abs(f) * V + np.abs(w0)
        adds += 2
    tol32 = EPS * (err + adds * reach)
    return W.reshape(shape), tol32.reshape(shape)


# ------------------------------------------------------------------ the same arithmetic in fp32, in the merge's operation order
def _chain32(u, d, mul):
    """sum_j (mul * u[:, j]) d[j, :] in fp32, ascending j"""
    acc = np.zeros((u.shape[0], d.shape[1]), np.float32)
    for j in range(u.shape[1]):
        acc = acc + (np.float32(mul) * u[:, j:j + 1]) * d[j:j + 1, :]
    return acc


def merge_fp32(w0, terms):
    """The merge as the device runs it, in float32 NumPy (products not fused): W before the rounding to the storage type."""
    shape = w0.shape
    N, K = int(shape[0]), int(np.prod(shape[1:]))
    w0 = np.asarray(w0, np.float32).reshape(N, K)
    f32 = lambda x: np.asarray(x, np.float32)
    active = [t for t in terms if _f32(t["s"]) != 0.0]
    plain = [t for t in active if t["kind"] == "pair" and t.get("magnitude") is None]
    total, first = w0, True
    if plain:
        acc = np.zeros((N, K), np.float32)
        for t in plain:
            u = f32(t["up"]).reshape(N, -1) * np.float32(t.get("scale", 1.0))
            d = f32(t["down"])
            for j in range(u.shape[1]):
                acc = acc + (np.float32(t["s"]) * u[:, j:j + 1]) * d.reshape(d.shape[0], K)[j:j + 1, :]
        total = w0 + acc
    for t in active:
        if any(t is q for q in plain):
            continue
        s, sc = np.float32(t["s"]), np.float32(t.get("scale", 1.0))
        if t["kind"] == "kron":
            w1, w2 = f32(t["up"]) * sc, f32(t["down"])
            w2 = w2.reshape(w2.shape[0], w2.shape[1], -1)
            D = ((s * w1)[:, None, :, None, None] * w2[None, :, None, :, :]).reshape(N, K)
        else:
            d = f32(t["down"])
            D = _chain32(f32(t["up"]).reshape(N, -1) * sc, d.reshape(d.shape[0], K), s)
            if t["kind"] == "hada":
                d2 = f32(t["down2"])
                D = D * _chain32(f32(t["up2"]).reshape(N, -1), d2.reshape(d2.shape[0], K), 1.0)
        m = t.get("magnitude")
        if m is not None:
            v = w0 + D
            ss = np.zeros((N, 1), np.float32)
            for k in range(K):
                ss = ss + v[:, k:k + 1] * v[:, k:k + 1]
            n = np.sqrt(ss)
            with np.errstate(divide="ignore", invalid="ignore"):
                f = np.where(n > 0, f32(m).reshape(N, 1) / n, np.float32(0)).astype(np.float32)
            D = f * v - w0
        total = total + D
    return total.reshape(shape)
