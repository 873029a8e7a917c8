"""Multi-window index maps of csrc/st_tail.hip (test infrastructure, CPU only): the context K / V of a sample in NW = ceil(Nk / 96)
windows of 96 keys, the ring schedule that carries them, and the online softmax across the windows.

tests/st_tail_emul.py restates the kernel's single-window maps and stays as it is; this file adds what the template parameter NW
of st_tail_kernel changes, with the same function names as the device code where there is one (steps_pair, steps_total, step_src,
st_tail_kv_pack_kernel -> kv_source / pack_kv).  NW = 1 reproduces st_tail_emul's pack_kv and the 9-step pair of the parent kernel.
"""
import numpy as np

from tests import st_tail_emul as E1

KWIN = 96                      # context keys per window
MAX_NW = 3                     # windows the kernel is instantiated for
KV_PAIR = 60                   # fragments per (head pair, window): [K h0 9][V h0 12][K h1 9][V h1 12][pad 18]
SF = 20                        # fragments per ring step
NT, KS, DH = E1.NT, E1.KS, E1.DH
STEPS_A, STEPS_CHUNK, STEPS_D = 10, 3, 10
WF_A, WF_PAIR = NT * KS, 120
WF_B = 4 * WF_PAIR


def windows(Nk):
    return (Nk + KWIN - 1) // KWIN


def steps_pair(nw):
    """ring steps of a head pair: 3 of q weights, 3 per window of K / V, 3 of attn2.to_out weights"""
    return 6 + 3 * nw


def steps_total(nw):
    return STEPS_A + 4 * steps_pair(nw) + E1.NCHUNK * STEPS_CHUNK + STEPS_D


def step_src(s, nw):
    """Pipe::step_src: ring step s -> ("w", first fragment of the weight stream) or ("kv", first fragment of the sample's
    [4][nw][KV_PAIR] K / V fragments).  Steps past the end re-read the last one."""
    sp = steps_pair(nw)
    s = min(s, steps_total(nw) - 1)
    if s < STEPS_A:
        return ("w", s * SF)
    if s < STEPS_A + 4 * sp:
        p, r = divmod(s - STEPS_A, sp)
        if r < 3:
            return ("w", WF_A + p * WF_PAIR + r * SF)
        if r < 3 + 3 * nw:
            return ("kv", p * nw * KV_PAIR + (r - 3) * SF)
        return ("w", WF_A + p * WF_PAIR + 60 + (r - 3 - 3 * nw) * SF)
    return ("w", WF_A + WF_B + (s - STEPS_A - 4 * sp) * SF)


def consumed(nw):
    """What the kernel's phases take from the ring, in order: a list of ("w" | "kv", fragment index), one entry per fragment."""
    out = [("w", f) for f in range(WF_A)]                                     # 1. attn1.to_out: 10 tiles x 20 k16 steps
    for p in range(4):
        out += [("w", WF_A + p * WF_PAIR + f) for f in range(60)]              # q of the pair: 3 tiles x 20
        for w in range(nw):                                                    # window w: K / V of head 0, head 1, padding
            out += [("kv", (p * nw + w) * KV_PAIR + f) for f in range(KV_PAIR)]
        out += [("w", WF_A + p * WF_PAIR + 60 + f) for f in range(60)]         # attn2.to_out: 2 heads x 10 tiles x 3
    n_c = E1.NCHUNK * STEPS_CHUNK * SF
    out += [("w", WF_A + WF_B + f) for f in range(n_c + NT * KS)]              # feed-forward stream, proj_out
    return out


def kv_source(pp, w, F, lane, j):
    """st_tail_kv_pack_kernel: element j of lane `lane` of fragment F of (head pair pp, window w) ->
    ("K" | "V", key, channel) of the sample's context K / V, or None (zero: padding, d >= 40).  Keys >= Nk are zeroed by the caller."""
    i, hk = lane & 31, lane >> 5
    if F >= 42:
        return None
    hl, q = divmod(F, 21)
    hd = 2 * pp + hl
    if q < 9:
        kt, ks = divmod(q, 3)
        key, d = KWIN * w + 32 * kt + E1.sigma(i), 16 * ks + 8 * hk + j
        return ("K", key, hd * DH + d) if d < DH else None
    dt, kk = divmod(q - 9, 6)
    d, key = 32 * dt + E1.sigma(i), KWIN * w + 32 * (kk >> 1) + 16 * hk + 8 * (kk & 1) + j
    return ("V", key, hd * DH + d) if d < DH else None


def pack_kv(K2, V2, Nk):
    """context K / V of one sample ([Nk][C] each) -> [4][NW][60][64][8] fragments"""
    nw = windows(Nk)
    out = np.zeros((4, nw, KV_PAIR, 64, 8), np.float64)
    for pp in range(4):
        for w in range(nw):
            for F in range(42):
                for lane in range(64):
                    for j in range(8):
                        src = kv_source(pp, w, F, lane, j)
                        if src is not None and src[1] < Nk:
                            out[pp, w, F, lane, j] = (K2 if src[0] == "K" else V2)[src[1], src[2]]
    return out


def attention_pair(qf, kv, Nk, scale):
    """The kernel's cross-attention of one head pair over nw windows.  qf [6][64][8]: the pair's q as B fragments (head hl owns steps
    3 hl .. 3 hl + 2); kv [nw][60][64][8].  Window by window, head 0 then head 1: S^T = K . q^T, the window's max joins the running
    max, O and the running sum are rescaled by exp(m_old - m_new), P = exp(S - m_new), O += V^T . P^T; O / sum after the last window.
    Returns the two heads' O as B fragments [2][3][64][8] (what attn2.to_out multiplies)."""
    nw = kv.shape[0]
    lane_hh = np.arange(64) >> 5
    O = np.zeros((2, 2, 64, 16))
    mrun = np.full((2, 64), -np.inf)
    lrun = np.zeros((2, 64))
    for w in range(nw):
        for hl in range(2):
            S = np.zeros((3, 64, 16))
            for kt in range(3):
                for ks in range(3):
                    E1.mfma(kv[w, hl * 21 + kt * 3 + ks], qf[3 * hl + ks], S[kt])
            key = KWIN * w + 32 * np.arange(3)[:, None, None] + 16 * lane_hh[None, :, None] + np.arange(16)[None, None, :]
            Sm = S * scale
            if w == nw - 1:                                   # keys >= Nk exist in the last window only
                Sm = np.where(key < Nk, Sm, -np.inf)
            else:
                assert (key < Nk).all()
            m = Sm.max(axis=(0, 2))
            m = np.maximum(m, np.roll(m, 32))
            m = np.maximum(m, mrun[hl])
            al = np.exp(mrun[hl] - m)                         # 0 in the first window (running max -inf), 1 where the max stayed
            Pm = np.exp(Sm - m[None, :, None])
            l = Pm.sum(axis=(0, 2))
            l = l + np.roll(l, 32)
            lrun[hl] = lrun[hl] * al + l
            O[hl] *= al[None, :, None]
            mrun[hl] = m
            pf = np.concatenate([E1.acc_to_bfrags(Pm[kt]) for kt in range(3)])
            for dt in range(2):
                for kk in range(6):
                    E1.mfma(kv[w, hl * 21 + 9 + dt * 6 + kk], pf[kk], O[hl, dt])
    of = np.zeros((2, 3, 64, 8))
    for hl in range(2):
        o = O[hl] / lrun[hl][None, :, None]
        of[hl] = np.concatenate([E1.acc_to_bfrags(o[0]), E1.acc_to_bfrags(o[1])[:1]])
    return of
