"""NumPy restatement of the engine's seeded noise (include/pdengine.h, "Seeded noise") and of the Euler ancestral rows.

Philox4x32-10 in integer arithmetic; u(r) in float32 exactly as the kernels form it; the Box-Muller radius and angle in fp64,
so the normals here carry only the fp64 rounding of log / sqrt / cos / sin: the reference the device's fp32 evaluation is
measured against."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
SH = np.uint64(32)
STREAMS = {"xt": 0, "step": 1, "vae": 2}
DIST_SEED = 20240229     # the seed of the distribution tests: the restatement alone passes all three checks (tests/test_rng_cpu.py)


def philox4x32_10(ctr, key):
    """ctr: four uint32 values or arrays (broadcast), key: two -> tuple of four uint64 arrays holding the uint32 outputs."""
    c0, c1, c2, c3 = (np.asarray(v, np.uint64) & MASK for v in ctr)
    k0, k1 = (np.asarray(v, np.uint64) & MASK for v in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2           # 32 x 32 -> 64 bits, no overflow
        n0 = (p1 >> SH) ^ c1 ^ k0
        n2 = (p0 >> SH) ^ c3 ^ k1
        c1, c3 = p1 & MASK, p0 & MASK
        c0, c2 = n0, n2
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def u01(r):
    """u(r) = (float)r * 2^-32 + 2^-33 in float32, in (0, 1]."""
    return np.asarray(r, np.uint64).astype(np.float32) * np.float32(2.0 ** -32) + np.float32(2.0 ** -33)


def normals(seed, sample, draw, stream, per_sample):
    """(z, radius), fp64 [per_sample]: the draws of one sample at (stream, draw) and the Box-Muller radius behind each."""
    st = STREAMS[stream] if isinstance(stream, str) else int(stream)
    nq = (int(per_sample) + 3) // 4
    q = np.arange(nq, dtype=np.uint64) & MASK
    r = philox4x32_10((q, np.uint64(int(sample) & 0xFFFFFFFF), np.uint64(draw), np.uint64(st)),
                      (np.uint64(int(seed) & 0xFFFFFFFF), np.uint64((int(seed) >> 32) & 0xFFFFFFFF)))
    z = np.empty((nq, 4), np.float64)
    rad = np.empty((nq, 4), np.float64)
    for h in (0, 1):
        u0 = u01(r[2 * h]).astype(np.float64)
        u1 = u01(r[2 * h + 1]).astype(np.float64)
        radius = np.sqrt(-2.0 * np.log(u0))
        ang = np.pi * (2.0 * u1)
        z[:, 2 * h], z[:, 2 * h + 1] = radius * np.cos(ang), radius * np.sin(ang)
        rad[:, 2 * h] = rad[:, 2 * h + 1] = radius
    return z.reshape(-1)[:per_sample], rad.reshape(-1)[:per_sample]


def randn(seed, sample_base, shape, stream="step", draw=0):
    """(z, radius) fp64 of shape `shape` = [B, ...]: what Engine.randn(shape, stream, draw) returns after set_rng(seed, sample_base)."""
    per = int(np.prod(shape[1:], dtype=np.int64))
    zs, rs = zip(*[normals(seed, (int(sample_base) + b) & 0xFFFFFFFF, draw, stream, per) for b in range(shape[0])])
    return np.stack(zs).reshape(shape), np.stack(rs).reshape(shape)


def euler_a_rows(alphas_cumprod, timesteps):
    """Rows [steps, 16] (fp64) of PD_LMS_EULER_A on the grid `timesteps` (sampling order), landing on sigma = 0."""
    ac = np.asarray(alphas_cumprod, np.float64)
    ts = [int(t) for t in timesteps]
    rows = np.zeros((len(ts), 16), np.float64)
    for i, t in enumerate(ts):
        a_from, sg_from = np.sqrt(ac[t]), np.sqrt(1.0 - ac[t])
        s_from = sg_from / a_from
        last = i + 1 == len(ts)
        a_to = 1.0 if last else np.sqrt(ac[ts[i + 1]])
        s_to = 0.0 if last else np.sqrt(1.0 - ac[ts[i + 1]]) / a_to
        s_up = np.sqrt(s_to ** 2 * (s_from ** 2 - s_to ** 2) / s_from ** 2)
        s_down = np.sqrt(s_to ** 2 - s_up ** 2)
        rows[i, 0], rows[i, 1], rows[i, 2] = a_from, sg_from, 16          # PD_LMS_F_STEP
        rows[i, 3], rows[i, 4] = a_to / a_from, a_to * (s_down - s_from)
        rows[i, 8], rows[i, 9] = 1.0 / a_from, -sg_from / a_from
        rows[i, 14] = 0.0 if last else a_to * s_up
    return rows
