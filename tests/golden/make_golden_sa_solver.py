"""Generate the SA-Solver golden vectors by IMPORTING THE REFERENCE (authoring container only).

Run:  python tests/golden/make_golden_sa_solver.py     (needs the reference checkout oracle/ref_import.py locates; writes tests/golden/t2i_sa_solver.npz)

From the reference's own ``diffusion.model.sa_solver`` (t2i/diffusion/model/sa_solver.py) on the CPU, built as
t2i/diffusion/sa_sampler.py:19-22,75-90 builds it (the wrapper class itself moves its buffer to a GPU): NoiseScheduleVP(
'discrete', alphas_cumprod=fp32 cumprod of the linear alphas) + model_wrapper(noise model, classifier-free guidance) +
SASolver(data prediction), driven by the analytic forward_with_dpmsolver-shaped model of tests/sa_step_cases.py on a
[1, 4, 8, 8] latent:
  * per trajectory of sa_step_cases.TRAJECTORIES (``return_intermediate=True``): the start latent, the 1 + S noise draws
    ``randn_like`` makes after ``torch.manual_seed``, every intermediate, the final sample, the model-input times seen;
  * direct calls of the four update functions (orders 1 - 4) and of get_coefficients_fn (orders 1 - 4) for tau in TAUS on
    the two TIME_LISTS, on seeded inputs;
  * get_time_steps for 'time', 'logSNR' and 'karras' at N = 5 and 25.
Only data is written; no reference source text.
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_import  # noqa: E402
import sa_step_cases as sc  # noqa: E402


def reference_solver(model=None, cfg_scale=sc.GUIDE):
    """The reference's SASolver as sa_sampler.py:19-22,75-88 builds it, with a zero text embedding."""
    ref_import.load_t2i()
    ref = importlib.import_module("diffusion.model.sa_solver")
    gd = importlib.import_module("diffusion.model.gaussian_diffusion")
    betas = torch.tensor(gd.get_named_beta_schedule("linear", 1000))
    alphas_cumprod = torch.as_tensor(np.cumprod(1.0 - betas, axis=0)).clone().detach().to(torch.float32)
    ns = ref.NoiseScheduleVP("discrete", alphas_cumprod=alphas_cumprod)
    y = torch.zeros(1, 1, 2, 4)
    model_fn = ref.model_wrapper(model, ns, model_type="noise", guidance_type="classifier-free", condition=y,
                                 unconditional_condition=y.clone(), guidance_scale=cfg_scale, model_kwargs={})
    return ref.SASolver(model_fn, ns, algorithm_type="data_prediction")


def reference_trajectory(name, seed=sc.SEED):
    """(intermediates [.., ...], final, model-input times seen) of the reference's own loop."""
    mode, steps, p, c, pc_mode, skip, eta, half = sc.TRAJECTORIES[name]
    calls = []
    solver = reference_solver(sc.analytic_model(half, calls))
    torch.manual_seed(seed)
    x, mid = solver.sample(mode=mode, x=sc.start_latent(seed), tau=sc.tau_window(eta), steps=steps, skip_type=skip,
                           skip_order=1, predictor_order=p, corrector_order=c, pc_mode=pc_mode, return_intermediate=True)
    return torch.stack([m.float() for m in mid]), x, torch.stack([t[0] for t in calls])


def reference_updates(solver, li, order, tau):
    """{function name: x_t} of the four updates and the coefficient vector, on time list ``li``."""
    prev, t = sc.TIME_LISTS[li]
    x, models, noise = sc.update_inputs(li)
    t_prev = [torch.tensor(v) for v in prev[-order:]]
    t = torch.tensor(t)
    out = {name: getattr(solver, name)(order, x, tau, models[-order:], t_prev, noise, t) for name in sc.UPDATES}
    lam = solver.noise_schedule.marginal_lambda
    lambda_list = [lam(t_prev[-(i + 1)]) for i in range(order)]
    out["get_coefficients_fn"] = torch.cat([torch.as_tensor(v, dtype=torch.float32).reshape(1) for v in
                                            solver.get_coefficients_fn(order, lam(t_prev[-1]), lam(t), lambda_list, tau)])
    return out


def main():
    out = {}
    for name, cfg in sc.TRAJECTORIES.items():
        mid, x, seen = reference_trajectory(name)
        assert torch.isfinite(mid).all() and torch.isfinite(x).all()
        key = "traj.%s." % name
        out[key + "z"] = sc.start_latent().numpy()
        out[key + "noise"] = sc.noise_stack(sc.SEED, cfg[1]).numpy()
        out[key + "mid"], out[key + "final"], out[key + "times"] = mid.numpy(), x.numpy(), seen.numpy()
    solver = reference_solver()
    for li in range(len(sc.TIME_LISTS)):
        for order in (1, 2, 3, 4):
            for ti, tau in enumerate(sc.TAUS):
                for name, v in reference_updates(solver, li, order, tau).items():
                    assert torch.isfinite(v).all(), (name, li, order, tau)
                    out["upd.%s.L%d.o%d.tau%d" % (name, li, order, ti)] = v.numpy()
    for skip in sc.SKIPS:
        for N in sc.GRID_N:
            out["grid.%s.N%d" % (skip, N)] = solver.get_time_steps(skip, 1.0, 1.0 / 1000, N, 1, "cpu").numpy()
    path = os.path.join(HERE, "t2i_sa_solver.npz")
    np.savez(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
