#!/usr/bin/env python3
"""Generate tests/golden/samplers_lms.npz from the REFERENCE's own PLMSSampler and DPM_Solver.

Runs only where a checkout of the reference project exists (--reference DIR); it uses the stubs and helpers of
tests/golden/make_golden.py and stores data only: inputs, the guided eps and model time of every evaluation, every state and
pred_x0 the samplers produced.  Nothing of the reference's source is stored.

Two model functions:
  * an analytic eps model (the closed form of make_golden.run_dpm_solver_case) -- PLMS at S in {3, 5, 10}, DPM-Solver++
    multistep at orders 1-3 x both solver types x lower_order_final on/off;
  * the TINY ControlNet + UNet of the other fixtures at 8 x 24 latents, B = 1, without CFG (plms.py:190 and model_wrapper's
    classifier-free branch torch.cat the conditioning, which the ControlLDM dict cannot take, so the dict goes in through a
    closure / guidance_type="uncond") -- PLMS S = 5, DPM-Solver++(2M) on an integer grid (S = 9: 999, 888, ..) and on the
    time-uniform fractional grid (S = 5: 999, 799.2, ..).
Everything runs in fp32, the reference's own precision.  For each trajectory `<tag>_f64diff` is the maximum difference
between the recorded states / pred_x0 and the same chain evaluated in fp64 (tests/lms_ref.py) from the recorded eps: the size
of the reference's own rounding, which the tests scale their tolerance from.

PLMS grids: the reference's make_ddim_timesteps yields arange(0, 1000, 1000 // S) + 1, which for S = 3 has a fourth entry,
1000, outside the schedule (IndexError in make_ddim_sampling_parameters).  So plms.make_ddim_timesteps is replaced for the
call by a function returning arange(S) * (1000 // S) + 1 -- the reference's own grid for S = 5 and 10 (asserted), its first
three points for S = 3 -- and PLMSSampler.sample / plms_sampling / p_sample_plms run unmodified on it.
DPM-Solver++ order 3 with lower_order_final: the reference raises on fewer than 15 steps (see main()), so that case has 16.
DPM-Solver++ integer grid: get_time_steps' float32 linspace does not give exact integers after model_wrapper's
(t - 1/N) * 1000, so the closure rounds the time it hands the network; the recorded time is the one the network saw.

Usage: python tests/golden/make_golden_samplers.py --reference DIR
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_golden as MG          # noqa: E402
from tests import lms_ref as L    # noqa: E402


def analytic_eps(A):
    def f(x, t_input):
        tc = t_input.to(x.dtype) / 1000.0 + 1.0 / 1000
        s = (0.3 + 0.6 * tc).reshape(-1, 1, 1, 1)
        return torch.tanh(torch.einsum("oc,bchw->bohw", A, x) * s) + 0.25 * x * (1.0 - s)
    return f


def plms_sampler(model):
    from ldm.models.diffusion.plms import PLMSSampler

    class CPUSampler(PLMSSampler):
        def register_buffer(self, name, attr):
            setattr(self, name, attr)
    return CPUSampler(model)


def run_plms(tag, model, eps_fn, S, x_T, res, ac64):
    """eps_fn(x, t) -> eps; model: the attributes PLMSSampler reads."""
    import ldm.models.diffusion.plms as plms_mod
    grid_asc = np.arange(S) * (1000 // S) + 1
    stock = plms_mod.make_ddim_timesteps
    if 1000 % S == 0:
        assert np.array_equal(stock(ddim_discr_method="uniform", num_ddim_timesteps=S, num_ddpm_timesteps=1000, verbose=False), grid_asc)
    calls = []

    def recording(x, t, c):
        e = eps_fn(x, t)
        calls.append((MG.t2n(x), int(t[0]), MG.t2n(e)))
        return e
    model.apply_model = recording
    plms_mod.make_ddim_timesteps = lambda **kw: grid_asc
    try:
        with torch.no_grad():
            samples, inter = plms_sampler(model).sample(S, x_T.shape[0], tuple(x_T.shape[1:]), conditioning=None, x_T=x_T,
                                                        log_every_t=1, verbose=False)
    finally:
        plms_mod.make_ddim_timesteps = stock
    assert len(calls) == S + 1
    grid = grid_asc[::-1].copy()
    xs = np.stack([MG.t2n(x) for x in inter["x_inter"]])          # x_T and the sample after every step
    preds = np.stack([MG.t2n(x) for x in inter["pred_x0"][1:]])
    eps = np.stack([c[2] for c in calls])
    cx, cp = L.plms_chain(ac64, grid, xs[0], eps)
    res.update({f"{tag}_grid": grid, f"{tag}_x": xs, f"{tag}_pred_x0": preds, f"{tag}_eps": eps,
                f"{tag}_eval_t": np.asarray([c[1] for c in calls], np.int64),
                f"{tag}_f64diff": np.float64(max(L.maxdiff(cx, xs[1:]), L.maxdiff(cp, preds)))})
    print(f"[golden] {tag}: {S} steps, {len(calls)} evaluations at {[c[1] for c in calls]}, f64diff {res[tag + '_f64diff']:.3e}")


def run_dpmpp(tag, eps_fn, S, order, solver_type, lof, x_T, res, ac32, ac64, round_times=False):
    from ldm.models.diffusion.dpm_solver.dpm_solver import NoiseScheduleVP, model_wrapper, DPM_Solver
    ns = NoiseScheduleVP("discrete", alphas_cumprod=ac32)
    calls = []

    def recording(x, t_input):
        t = torch.round(t_input) if round_times else t_input
        e = eps_fn(x, t)
        calls.append((MG.t2n(x), float(t[0]), MG.t2n(e)))
        return e
    solver = DPM_Solver(model_wrapper(recording, ns, model_type="noise", guidance_type="uncond"), ns, predict_x0=True)
    m_rec = []
    inner = solver.data_prediction_fn

    def data_pred(x, t):
        m = inner(x, t)
        m_rec.append(MG.t2n(m))
        return m
    solver.data_prediction_fn = data_pred
    with torch.no_grad():
        x = solver.sample(x_T.clone(), steps=S, t_start=1.0, t_end=1.0 / 1000, order=order, skip_type="time_uniform",
                          method="multistep", lower_order_final=lof, denoise_to_zero=False, solver_type=solver_type)
        ts = solver.get_time_steps(skip_type="time_uniform", t_T=1.0, t_0=1.0 / 1000, N=S, device=x_T.device)
    assert len(calls) == S and len(m_rec) == S
    land = float(((ts[-1] - 1.0 / 1000) * 1000.0).clamp(min=0.0))
    mt = np.asarray([c[1] for c in calls] + [round(land) if round_times else land], np.float64)
    xs = np.stack([c[0] for c in calls] + [MG.t2n(x)])            # the state at every evaluation and the final one
    eps = np.stack([c[2] for c in calls])
    preds = np.stack(m_rec)
    al, sg, _ = L.vp_points(ac64, mt)
    cx, cm = L.dpmpp_chain(al, sg, xs[0], eps, order, solver_type, lof and S < 15)
    res.update({f"{tag}_model_times": mt, f"{tag}_x": xs, f"{tag}_pred_x0": preds, f"{tag}_eps": eps,
                f"{tag}_order": np.int64(order), f"{tag}_taylor": np.int64(solver_type == "taylor"), f"{tag}_lof": np.int64(bool(lof)),
                f"{tag}_f64diff": np.float64(max(L.maxdiff(cx, xs[1:]), L.maxdiff(cm, preds)))})
    print(f"[golden] {tag}: {S} evaluations at {np.round(mt, 3).tolist()}, f64diff {res[tag + '_f64diff']:.3e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, metavar="DIR", help="checkout of the reference project")
    args = ap.parse_args()
    MG.REF = os.path.abspath(args.reference)
    MG.install_stubs()
    sys.path.insert(0, MG.REF)
    os.chdir(MG.REF)
    from prompt_diffusion_amd import weights as W
    torch.manual_seed(0)
    torch.set_num_threads(8)
    cfg = W.TINY
    ac64 = L.alphas_cumprod64(cfg.linear_start, cfg.linear_end, cfg.timesteps)
    res = {}
    # ---- analytic eps model
    g = np.random.default_rng(11)
    x_T = torch.from_numpy(g.standard_normal((1, 4, 8, 8)).astype(np.float32))
    A = torch.from_numpy((g.standard_normal((4, 4)) * 0.3).astype(np.float32))
    res["an_A"] = A.numpy()
    f = analytic_eps(A)
    model, _, _ = MG.build_reference(cfg, W)     # the schedule buffers PLMSSampler reads (and, below, the TINY networks)
    net_apply = model.apply_model
    ac32 = model.alphas_cumprod
    for S in (3, 5, 10):
        run_plms(f"an_plms_s{S}", model, f, S, x_T, res, ac64)
    for order in (1, 2, 3):
        for st in ("dpm_solver", "taylor"):
            for lof in (True, False):
                # order 3 with lower_order_final on fewer than 15 steps cannot run in the reference: its second-order update
                # unpacks a two-entry history and the order-3 loop hands it three (dpm_solver.py:740, :1066).  That case runs
                # at 16 steps, where the reference's own rule (steps < 15, :1062) leaves the order alone.
                S = 16 if (order == 3 and lof) else 6
                run_dpmpp(f"an_dpmpp_o{order}_{st}_lof{int(lof)}", f, S, order, st, lof, x_T, res, ac32, ac64)
    # ---- the TINY networks, 8 x 24, B = 1, no CFG
    B, h, w = 1, 8, 24
    inp = W.synth_inputs(cfg, B, h, w)
    tt = {k: torch.from_numpy(v) for k, v in inp.items()}
    cond = {"c_crossattn": [tt["ctx_cond"]], "example_pair": [tt["pair"]], "query": [tt["query"]]}
    res["tiny_shape"] = np.asarray([B, h, w], np.int64)

    def net(x, t):
        tv = t if t.dtype.is_floating_point else t
        return net_apply(x, tv.expand(x.shape[0]) if tv.dim() else tv.reshape(1).expand(x.shape[0]), cond)
    run_plms("tiny_plms_s5", model, net, 5, tt["x_T"], res, ac64)
    run_dpmpp("tiny_dpmpp_int_s9", net, 9, 2, "dpm_solver", True, tt["x_T"], res, ac32, ac64, round_times=True)
    run_dpmpp("tiny_dpmpp_frac_s5", net, 5, 2, "dpm_solver", True, tt["x_T"], res, ac32, ac64)
    out = os.path.join(HERE, "samplers_lms.npz")
    np.savez_compressed(out, **res)
    print(f"[golden] samplers_lms.npz: {len(res)} arrays, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
