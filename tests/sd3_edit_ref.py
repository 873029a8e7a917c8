"""NumPy float32 restatement of the SD3 img2img / inpainting loop (diffusers' StableDiffusion3Img2ImgPipeline and the 16-channel path of
StableDiffusion3InpaintPipeline; diffusers is absent, so this restates the arithmetic of include/pdengine.h, pd_sd3_loop_args):

  truncation   t_start = int(max(n - min(n * strength, n), 0)); the loop runs on sig[t_start:]
  start state  x = sig_0 * eps + (1 - sig_0) * z0                         (FlowMatchEulerDiscreteScheduler.scale_noise)
  blend        x = (1 - m) * k_i + m * x',  k_i = (1 - sig_{i+1}) * z0 + sig_{i+1} * eps     after the Euler update x' of step i

Every operation is one float32 operation in the written order.  The loop itself runs over oracle/sd3_oracle.py forwards; controlnet_keep is
computed over the remaining steps.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle import sd3_oracle as O

F32 = np.float32
ONE = F32(1.0)


def t_start(n, strength):
    if not 0.0 <= strength <= 1.0:
        raise ValueError(f"strength {strength} outside [0, 1]")
    t = int(max(n - min(n * strength, n), 0))
    if n - t < 1:
        raise ValueError(f"strength {strength} leaves no step of {n}")
    return t


def truncate(sig, strength):
    """sig[0..n] (last 0) -> the kept tail sig[t_start:]"""
    sig = np.asarray(sig, F32)
    return sig[t_start(len(sig) - 1, strength):]


def start_state(sig0, eps, z0):
    s = F32(sig0)
    return (s * eps.astype(F32) + (ONE - s) * z0.astype(F32)).astype(F32)


def known(sig_next, z0, eps):
    s = F32(sig_next)
    return ((ONE - s) * z0.astype(F32) + s * eps.astype(F32)).astype(F32)


def blend(m, k, x):
    m = np.asarray(m, F32)
    return ((ONE - m) * k + m * x).astype(F32)


def keep_steps(n, start=0.0, end=1.0):
    return [1.0 - float(i / n < start or (i + 1) / n > end) for i in range(n)]


def oracle_velocity(sd, cfg, ctx, ctx_neg, pooled, pooled_neg, cond, pair, guidance, scale=1.0):
    """The guided velocity of one step as oracle.sample computes it: (x, sigma, keep) -> v [B, C, H, W]."""
    def f(x, sigma, keep):
        B = x.shape[0]
        if guidance > 1.0:
            t = np.full((2 * B,), F32(sigma) * F32(1000.0), F32)
            xi = np.concatenate([x, x])
            cc, pp = np.concatenate([ctx_neg, ctx]), np.concatenate([pooled_neg, pooled])
            cn, pr = np.concatenate([cond, cond]), np.concatenate([pair, pair])
        else:
            t = np.full((B,), F32(sigma) * F32(1000.0), F32)
            xi, cc, pp, cn, pr = x, ctx, pooled, cond, pair
        cp = np.zeros_like(pp) if cfg.force_zeros_for_pooled_projection else pp
        ctl = O.controlnet_forward(sd, cfg, xi, t, cc, cp, cn, pr, scale * keep)
        v = O.transformer_forward(sd, cfg, xi, t, cc, pp, ctl)
        if guidance > 1.0:
            v = v[:B] + F32(guidance) * (v[B:] - v[:B])
        return v.astype(F32)
    return f


def sample(velocity, sig, z0, eps, mask=None, guidance_start=0.0, guidance_end=1.0):
    """The edited loop on the kept grid sig[0..n] (already truncated): start state, then per step the Euler update and the blend."""
    sig = np.asarray(sig, F32)
    n = len(sig) - 1
    keep = keep_steps(n, guidance_start, guidance_end)
    x = start_state(sig[0], eps, z0)
    for i in range(n):
        v = velocity(x, sig[i], keep[i])
        x = (x + (sig[i + 1] - sig[i]) * v).astype(F32)
        if mask is not None:
            x = blend(mask, known(sig[i + 1], z0, eps), x)
    return x
