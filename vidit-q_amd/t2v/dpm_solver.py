"""DPM-Solver++ scheduler of the t2v sampling loop: the second entry of the reference's OpenSORA scheduler registry.

Mirrors t2v/opensora/schedulers/dpms/__init__.py (``DMP_SOLVER.sample`` :16-41, ``forward_with_dpmsolver`` :44-50,
``DPMS(...)`` dpms/dpm_solver.py:1537-1570): 20-step multistep DPM-Solver++ of order 2 with 'time_uniform' spacing,
classifier-free guidance on all four eps channels with ONE joint (uncond | cond) forward of 2n samples, the learned-sigma
half of the model output dropped by ``chunk(2, dim=1)[0]``.

The solver is t2i/dpm_solver.py's DPMSolverPP: schedule, updates, ``multistep_rows`` and the eager loop are used from
there, nothing is restated.  The reference's t2v solver file differs from its t2i one in ONE rule, which lives in
``lower_order_final`` below.  What is specific to video:
  * ``cfg_split=True`` (this package's extension, for plans whose grids were calibrated per branch): two forwards of n
    samples through iddpm.model_forward_pair - cond, then uncond, with the same mask - and guidance on the two outputs;
  * the host knows every model-input time and hands it to a QuantModel as ``timestep_id``, so no forward reads ``t[0]``
    back.  (It is the fp32 value (t - 1/N) * 1000 the reference's ``t[0].item()`` returns: a plan's time ranges have to
    cover it as they have to there);
  * the fused route (``fused=True`` or VQ_T2V_DPM_FUSED=1, off by default): per model call ``forward(patch_major=True)``
    once (joint) or twice (split) and one ops.cfg_dpmpp_step_patch, which reads final_layer's output where the model
    left it - no unpatchify copy, no fp32 cast, no ``torch.cat([x, x])`` - and writes the next forward's input in the
    model's dtype.  Bit-identical to the eager expressions on the same device.  ``step_graph`` is its one-graph form
    (graph.VideoDPMStepGraph).
"""
from __future__ import annotations

from functools import partial

import torch

from ..t2i.dpm_solver import DPMSolverPP, _switch
from .iddpm import _accepts_timestep_id, model_forward_pair, patch_forward_pair

_T2V_DPM_FUSED = _switch("VQ_T2V_DPM_FUSED", False)   # the patch-major step behind each model call


def lower_order_final(steps: int) -> bool:
    """The one rule in which the reference's t2v solver differs from its t2i one (dpms/dpm_solver.py:1419-1423 against
    t2i/diffusion/model/dpm_solver_sigma.py:1224-1226): the last steps drop to the lower orders only when there are fewer
    than 10 steps, so a 20-step run ends with a second-order update."""
    return steps < 10


def forward_with_dpmsolver(model, x, timestep, y, **kwargs):
    """dpms/__init__.py:44-50: the noise half of the model output (DPM-Solver needs no variance prediction)."""
    return model.forward(x, timestep, y, **kwargs).chunk(2, dim=1)[0]


class VideoDPMSolverPP(DPMSolverPP):
    """DPMSolverPP around an STDiT ``net``: the forwards of one model call (joint or split, with ``timestep_id``) and the
    patch-major fused route.  Every update, coefficient and the loop itself are the base class's."""

    def __init__(self, net, condition, uncondition, cfg_scale, model_kwargs=None, cfg_split=False):
        super().__init__(partial(forward_with_dpmsolver, net), condition, uncondition, cfg_scale, model_kwargs)
        self.net, self.cfg_split = net, bool(cfg_split)
        self._takes_id = _accepts_timestep_id(net)
        self.model_input_dtype = getattr(net, "dtype", torch.float32)

    def _noise(self, x, t_cont):
        t_val = self._t_val(t_cont)
        if self._takes_id:
            self.model_kwargs["timestep_id"] = t_val
        if not self.cfg_split or self.cfg_scale == 1.0 or self.uncondition is None:
            return super()._noise(x, t_cont)
        t = torch.full((x.shape[0],), t_val, dtype=torch.float32, device=x.device)
        extra = {k: v for k, v in self.model_kwargs.items() if k not in ("mask", "timestep_id")}
        cond, uncond = model_forward_pair(self.net, x, t, self.condition, self.uncondition, self.model_kwargs.get("mask"),
                                          True, t_val, extra)
        return self._guide(torch.cat([uncond.chunk(2, dim=1)[0], cond.chunk(2, dim=1)[0]]))

    # ---- the fused route
    def _fused_wanted(self, x, method, fused):
        if fused is None:
            fused = _T2V_DPM_FUSED
        return bool(fused) and method == "multistep" and self.cfg_scale != 1.0 and self.uncondition is not None and x.is_cuda

    def _forward_patch(self, xm, t, t_val, side=None):
        """(eps_u, eps_c): final_layer's output for the uncond and the cond samples.  Joint: the halves of one
        (uncond | cond) forward of ``xm`` [2n, ...]; split: cond, then uncond, each on ``xm`` [n, ...] - the uncond chain on
        the stream ``side`` when one is given (graph.VideoDPMStepGraph forks it as graph.StepGraph does)."""
        kw = {k: v for k, v in self.model_kwargs.items() if k != "timestep_id"}
        if self._takes_id:
            kw["timestep_id"] = t_val
        if not self.cfg_split:
            return patch_forward_pair(self.net, xm, t, self._joint_text(), False, kw)
        eps_c, eps_u = patch_forward_pair(self.net, xm, t, (self.condition, self.uncondition), True, kw, side=side)
        return eps_u, eps_c

    def _eager_eps(self, pair):
        """The (uncond | cond) noise tensor of the eager route from a patch-major pair (a refused first model output)."""
        return torch.cat([self.net.unpatchify(e).to(torch.float32).chunk(2, dim=1)[0] for e in pair])

    def _multistep_fused(self, x, ts, args, step_callback):
        """DPMSolverPP._multistep_fused with the patch-major forwards and step.  Returns (x, None), or (None, eps) when
        ops.cfg_dpmpp_step_patch_ok refuses the first model output: the caller goes on eagerly from it."""
        from .. import ops
        from ..t2i.fused_loop import device_table, fused_loop
        n, steps, order = x.shape[0], args[0], args[1]
        copies = 1 if self.cfg_split else 2
        patch = tuple(self.net.patch_size)
        x = x.float().contiguous() if x.dtype != torch.float32 or not x.is_contiguous() else x
        xm = torch.cat([x] * copies).to(self.model_input_dtype)
        hist = torch.empty((3, x.numel()), dtype=torch.float32, device=x.device)
        t_vals = [self._t_val(v) for v in ts[:steps]]
        t = torch.full((copies * n,), t_vals[0], dtype=torch.float32, device=x.device)
        call = [0]

        def forward(xm, t):
            k = call[0]
            call[0] += 1
            return self._forward_patch(xm, t[:copies * n], t_vals[k])

        def table(eps, x):
            if not ops.cfg_dpmpp_step_patch_ok(eps[0], eps[1], x, patch):
                return None
            return device_table(self._tables, (args, self.cfg_scale, str(x.device), n),
                                lambda: self.multistep_rows(*args), x.device, n)

        def step(k, eps, x, rows):
            # a fresh x_out per step: what a step_callback was handed is never written again
            x = ops.cfg_dpmpp_step_patch(eps[0], eps[1], x, hist, rows, k, patch, x_model=xm)
            if step_callback is not None and k + 1 >= order:
                step_callback(k + 1, x)
            return x

        x_f, eps0 = fused_loop(steps, x, xm, t, forward, table, step)
        return (x_f, None) if x_f is not None else (None, self._eager_eps(eps0))

    def step_graph(self, x, steps=20, order=2, warmup=2):
        """The counter form of the fused loop: {forward(s), patch-major step, counter advance} captured as HIP graphs - one
        per smooth-quant time range the schedule visits - and replayed ``steps`` times; ``.run(x)`` samples."""
        from ..graph import VideoDPMStepGraph
        assert self.cfg_scale != 1.0 and self.uncondition is not None, "the fused step is the guided one"
        rows = self.multistep_rows(steps, order, "time_uniform", None, None, lower_order_final(steps), "dpmsolver")
        ts = self.time_steps("time_uniform", self.ns.T, 1.0 / self.ns.total_N, steps)
        return VideoDPMStepGraph(self, x, rows, [self._t_val(v) for v in ts[:steps]], warmup=warmup)


class DMP_SOLVER:
    """dpms/__init__.py:10-41 (the reference's spelling; ``DPM_SOLVER`` is the same class)."""

    def __init__(self, num_sampling_steps=None, cfg_scale=4.0):
        self.num_sampling_steps = num_sampling_steps
        self.cfg_scale = cfg_scale

    def solver(self, model, text_encoder, prompts, additional_args=None, cfg_split=None) -> VideoDPMSolverPP:
        """The solver ``sample`` runs: DPMS(partial(forward_with_dpmsolver, model), condition=y, uncondition=null_y,
        cfg_scale, model_kwargs) with the mask of ``text_encoder.encode`` passed through."""
        if getattr(model, "timestep_wise_mp", False):
            raise NotImplementedError("timestep_wise_mp: the reference switches precision in the DDIM loop only")
        n = len(prompts)
        model_args = text_encoder.encode(prompts)
        y = model_args.pop("y")
        null_y = text_encoder.null(n)
        if additional_args is not None:
            model_args.update(additional_args)
        return VideoDPMSolverPP(model, y, null_y, self.cfg_scale, model_args, bool(cfg_split))

    @torch.no_grad()
    def sample(self, model, text_encoder, z_size, prompts, device, additional_args=None, init_noise=None, generator=None,
               cfg_split=None, fused=None, step_callback=None):
        """Returns the n samples [n, *z_size] fp32.  ``cfg_split``: None / False the reference's joint forward, True two
        forwards of n samples.  ``fused``: None reads the VQ_T2V_DPM_FUSED switch.  ``step_callback(i, x)`` as in
        DPMSolverPP.sample."""
        solver = self.solver(model, text_encoder, prompts, additional_args, cfg_split)
        n = len(prompts)
        z = torch.randn(n, *z_size, device=device, generator=generator) if init_noise is None else init_noise.to(device)
        steps = self.num_sampling_steps
        return solver.sample(z, steps=steps, order=2, skip_type="time_uniform", method="multistep",
                             lower_order_final=lower_order_final(steps), fused=fused, step_callback=step_callback)

    def step_graph(self, model, text_encoder, z_size, prompts, device, additional_args=None, cfg_split=None, warmup=2):
        """graph.VideoDPMStepGraph of this configuration; ``.run(z)`` samples from a start latent [n, *z_size]."""
        solver = self.solver(model, text_encoder, prompts, additional_args, cfg_split)
        z = torch.zeros(len(prompts), *z_size, device=device)
        return solver.step_graph(z, steps=self.num_sampling_steps, order=2, warmup=warmup)


DPM_SOLVER = DMP_SOLVER
