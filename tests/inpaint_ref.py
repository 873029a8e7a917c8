"""NumPy restatement of diffusers' img2img / inpainting loop logic for a 4-channel UNet (StableDiffusionControlNetImg2Img /
Inpaint pipelines): get_timesteps, the mask processor, add_noise and the per-step blend, written out independently of the
package so that the tests check the pipelines and the engine against it.  All latent arithmetic is fp32."""
import numpy as np


def get_timesteps(timesteps, strength, order=1):
    """(the truncated grid, the begin index)"""
    S = len(timesteps)
    init_timestep = min(int(S * strength), S)
    t_start = max(S - init_timestep, 0)
    return list(timesteps[t_start * order:]), t_start * order


def alphas_cumprod_f32(cfg):
    T = cfg.timesteps
    s0, s1 = np.sqrt(cfg.linear_start), np.sqrt(cfg.linear_end)
    betas = np.array([(s1 if i == T - 1 else s0 + (s1 - s0) / (T - 1) * i) ** 2 for i in range(T)], np.float64)
    return np.cumprod(1.0 - betas).astype(np.float32)


def add_noise(ac32, z0, eps, t):
    """scheduler.add_noise(original_samples, noise, t) with the fp32 table: sqrt(abar) * x0 + sqrt(1 - abar) * noise"""
    a = ac32[int(t)]
    return np.sqrt(a) * z0 + np.sqrt(np.float32(1.0) - a) * eps


def blend(known, latents, mask):
    return (np.float32(1.0) - mask) * known + mask * latents


def known_after_step(ac32, z0, eps, ts, i):
    """init_latents_proper after step i of the grid ts: z0 noised to the next step's timestep, z0 itself after the last"""
    return z0 if i == len(ts) - 1 else add_noise(ac32, z0, eps, ts[i + 1])


def process_mask(mask01, batch_size, vae_scale_factor=8):
    """mask [Bm, 1, H, W] in [0, 1] at the image size -> binarized, F.interpolate(size=(H/8, W/8)) (nearest), repeated"""
    m = np.asarray(mask01, np.float32).copy()
    m[m < 0.5] = 0.0
    m[m >= 0.5] = 1.0
    H, W = m.shape[-2:]
    h, w = H // vae_scale_factor, W // vae_scale_factor
    rows = np.floor(np.arange(h) * (H / h)).astype(int)
    cols = np.floor(np.arange(w) * (W / w)).astype(int)
    m = m[:, :, rows][:, :, :, cols]
    return np.tile(m, (batch_size // m.shape[0], 1, 1, 1))


def start_latents(ac32, z0, eps, ts, inpaint, strength, latents_given=False):
    """img2img: add_noise(z0, eps, t_first) always; inpainting: the noise itself at strength 1 or for given latents"""
    if inpaint and (strength == 1.0 or latents_given):
        return eps
    return add_noise(ac32, z0, eps, ts[0])


def run_loop(step, ac32, z0, eps, mask, ts, x_start):
    """diffusers' denoising loop around a scheduler step: `step(i, x) -> x` is one plain update; the 4-channel inpainting
    blend follows every step.  Returns the latents after every step."""
    x, out = x_start, []
    for i in range(len(ts)):
        x = step(i, x)
        if mask is not None:
            x = blend(known_after_step(ac32, z0, eps, ts, i), x, mask)
        out.append(x)
    return out
