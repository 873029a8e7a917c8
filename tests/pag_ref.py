"""NumPy restatement of perturbed-attention guidance (PAG) on the oracle.  Pure NumPy on the CPU, no engine import: shared by
test_pag_cpu.py (the inputs of the GPU tests have teeth) and test_pag_gpu.py.

Restated from diffusers' PAGMixin / PAGCFGIdentitySelfAttnProcessor2_0 (diffusers is not installed where the tests run, so parity with it
is unpinned): the perturbed branch is the conditional branch -- same latent, timestep, context, example pair, query and ControlNet
residuals -- whose self-attention (attn1) in the chosen UNet blocks returns to_out(to_v(norm1(h))), bias included, instead of
to_out(softmax(q k^T) v).  oracle.pd_oracle.cross_attention is wrapped at run time (pag_active), the way ip_adapter_ref.ip_active wraps
it: Net.prefix tells the UNet from the ControlNet (never perturbed), the layer prefix tells attn1 of a chosen block, and only the chosen
sample rows change.  It wraps whatever cross_attention is current, so it composes with ip_active in either order.

The evaluation is the plain one: the batch is [uncond ; cond ; perturbed] (or [cond ; perturbed]) from the first layer on, with the
conditional inputs and residuals doubled.  Guidance, fp32 with every operation rounded on its own:
    e = (e_u + s (e_c - e_u)) + p (e_c - e_p)      under CFG,          e = e_c + p (e_c - e_p)      without
p = scale, or max(scale - adaptive (1000 - t), 0) in double, where scale and adaptive are the fp32 values the C ABI carries."""
import contextlib

import numpy as np

from oracle import pd_oracle as O

F32 = np.float32
UNET = "model.diffusion_model."
ATTN1 = "transformer_blocks.0.attn1."


def block_prefixes(cfg, W):
    """SpatialTransformer prefixes relative to the UNet in the engine's block order: encoder, decoder, middle block
    (prompt_diffusion_amd.ip_adapter.block_prefixes restated on the layouts, so this module imports no engine code)."""
    enc = [f"input_blocks.{i}.1." for i, b in enumerate(W.encoder_layout(cfg)) if b["attn"]]
    dec = [f"output_blocks.{i}.1." for i, b in enumerate(W.decoder_layout(cfg)) if b["attn"]]
    return enc + dec + ["middle_block.1."]


@contextlib.contextmanager
def pag_active(prefixes, rows):
    """While it lives, attn1 of the UNet blocks under `prefixes` (relative SpatialTransformer prefixes) is the identity attention for
    the sample rows `rows` (a slice or an index array): to_out(to_v(x))."""
    prefixes = set(prefixes)
    orig = O.cross_attention

    def cross_attention(p, pre, x, context=None, heads=8):
        out = orig(p, pre, x, context, heads)
        if context is not None or p.prefix != UNET or not pre.endswith(ATTN1) or pre[:-len(ATTN1)] not in prefixes:
            return out
        out = np.array(out, copy=True)
        v = O.linear(x[rows], p(pre + "to_v.weight"))
        out[rows] = O.linear(v, p(pre + "to_out.0.weight"), p(pre + "to_out.0.bias"))
        return out

    O.cross_attention = cross_attention
    try:
        yield
    finally:
        O.cross_attention = orig


def spatial_transformer_pag(sd, prefix, x, ctx, heads, n_perturbed):
    """One block of the UNet (absolute prefix under model.diffusion_model.) with the last n_perturbed samples perturbed."""
    assert prefix.startswith(UNET)
    rel = prefix[len(UNET):]
    B = x.shape[0]
    with pag_active([rel], slice(B - n_perturbed, B)):
        return O.spatial_transformer(O.Net(sd, UNET), rel, x, ctx, heads)


def pag_scale_at(scale, adaptive, t):
    """p_i of an evaluation at timestep t."""
    s, a = float(F32(scale)), float(F32(adaptive))
    if a == 0.0:
        return F32(s)
    return F32(max(s - a * (1000.0 - float(t)), 0.0))


def guide(e_u, e_c, e_p, s, p):
    """The guided eps; e_u None: no CFG.  p == 0 is the two-term formula bit for bit (the term is skipped, as the kernel skips it)."""
    e = e_c if e_u is None else e_u + F32(s) * (e_c - e_u)
    if F32(p) != 0:
        e = e + F32(p) * (e_c - e_p)
    return e.astype(F32)


def eps_branches(sd, cfg, lay, W, x, t, cond, uncond, blocks, guess_mode=False, control_scales=None, only_mid_control=False):
    """(e_u or None, e_c, e_p) of the plain [u ; c ; p] evaluation at latents x [B, ...], integer timestep t.  cond / uncond: dicts with
    c_crossattn, example_pair, query (uncond None: no CFG); blocks: engine block indices of the perturbed layer set (empty: e_p = e_c).
    guess_mode: the unconditional third gets zero residuals, the perturbed one the conditional residuals."""
    B = x.shape[0]
    parts = ([uncond] if uncond is not None else []) + [cond, cond]
    n = len(parts)
    x_in = np.concatenate([x] * n)
    t_in = np.full((n * B,), int(t), np.int64)
    c_in = {k: np.concatenate([p[k] for p in parts]) for k in ("c_crossattn", "example_pair", "query")}
    control = O.controlnet_forward(sd, cfg, lay, x_in, t_in, c_in["example_pair"], c_in["query"], c_in["c_crossattn"])
    scales = [1.0] * len(control) if control_scales is None else control_scales
    control = [c * F32(s) for c, s in zip(control, scales)]
    if guess_mode and uncond is not None:
        for c in control:
            c[:B] = 0
    pre = block_prefixes(cfg, W)
    with pag_active([pre[j] for j in blocks], slice((n - 1) * B, n * B)):
        out = O.controlled_unet_forward(sd, cfg, lay, x_in, t_in, c_in["c_crossattn"], control, only_mid_control)
    if uncond is not None:
        return out[:B], out[B:2 * B], out[2 * B:]
    return None, out[:B], out[B:]


def ddim_pag(sd, cfg, lay, W, S, x_T, cond, uncond, cfg_scale, pag_scale, blocks, adaptive=0.0, steps_limit=None, guess_mode=False):
    """The DDIM loop (eta 0) of ddim_hacked.py on O.make_schedule with the guidance above: list of the latents after every step."""
    sched = O.make_schedule(S, 0.0, cfg.timesteps, cfg.linear_start, cfg.linear_end)
    n = len(sched["ddim_timesteps"])
    x, out = x_T, []
    for i, step in enumerate(np.flip(sched["ddim_timesteps"])):
        if steps_limit is not None and i >= steps_limit:
            break
        index = n - 1 - i
        e_u, e_c, e_p = eps_branches(sd, cfg, lay, W, x, int(step), cond, uncond, blocks, guess_mode)
        e = guide(e_u, e_c, e_p, cfg_scale, pag_scale_at(pag_scale, adaptive, int(step)))
        a_t, a_prev = sched["ddim_alphas"][index], sched["ddim_alphas_prev"][index]
        pred_x0 = (x - sched["ddim_sqrt_one_minus_alphas"][index] * e) / np.sqrt(a_t)
        x = (np.sqrt(a_prev) * pred_x0 + np.sqrt(F32(1.0) - a_prev - sched["ddim_sigmas"][index] ** 2) * e).astype(F32)
        out.append(x)
    return out
