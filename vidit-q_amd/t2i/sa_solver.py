"""SA-Solver (stochastic Adams predictor-corrector) driver of the t2i sampling loop: ``--sampling_algo sa-solver`` of the
reference's t2i script (quant_txt2img.py:167-181).

Restates t2i/diffusion/model/sa_solver.py for ``algorithm_type="data_prediction"`` and its wrapper
t2i/diffusion/sa_sampler.py: NoiseScheduleVP('discrete', alphas_cumprod=...) :7-165 (dpm_solver.NoiseScheduleVP
.from_alphas_cumprod), model_wrapper :173-322 (dpm_solver.GuidedModel), SASolver.{data_prediction_fn :377-386,
get_time_steps :398-418, get_coefficients_exponential_negative :426, get_coefficients_exponential_positive :449,
lagrange_polynomial_coefficient :478, get_coefficients_fn :541, adams_bashforth_update :562, adams_moulton_update :602,
adams_bashforth_update_few_steps :644, adams_moulton_update_few_steps :700, sample_few_steps :755, sample_more_steps :911,
sample :1066}; SASolverSampler sa_sampler.py:10-94.

Where things run: every schedule quantity, tau(t), the Lagrange and exponential-integral coefficients are one-element fp32
torch tensors on the HOST, computed with the reference's own expressions in its order (it computes them on the device, with
two host syncs per step for tau); what meets the latent is a one-element fp32 tensor on the latent's device, so the type
promotion is the reference's: ``sigma_t * noise`` of an fp16 model output is an fp32 product and the division by alpha_t is
a tensor / tensor division.

The fused route (``fused=True`` or VQ_SA_FUSED=1; off by default): for 'few_steps', PEC, predictor order <= 2, corrector
order 1 - 2, guided, on GPU tensors, ONE launch of ops.cfg_sa_step behind each model call does guidance + x0 + the
corrector of this step + the predictor of the next (``pec_rows`` is its coefficient table); bit-identical to the eager
expressions, which every other configuration runs.  Not built (NotImplementedError): ``algorithm_type="noise_prediction"``,
``correcting_x0_fn`` (dynamic thresholding) and ``correcting_xt_fn``.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np
import torch

from .dpm_solver import GuidedModel, NoiseScheduleVP, _switch, linear_betas

_SA_FUSED = _switch("VQ_SA_FUSED", False)            # guidance + x0 + corrector + next predictor in one launch


def _on(s: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """The host scalar ``s`` (one-element fp32) where ``x`` lives, still a one-element 1-D tensor: written by a fill
    kernel (a copy of a host tensor would make the host wait for the queued GPU work)."""
    if s.device == x.device:
        return s
    return torch.full((1,), float(s), dtype=s.dtype, device=x.device)


class SASolver(GuidedModel):
    """``SASolver(model_wrapper(model, ns, ...), ns, algorithm_type="data_prediction")`` on the schedule of
    sa_sampler.py:19-22,75."""

    def __init__(self, model: Callable, condition: torch.Tensor, uncondition: Optional[torch.Tensor], cfg_scale: float,
                 model_kwargs: Optional[dict] = None, diffusion_steps: int = 1000, algorithm_type="data_prediction",
                 correcting_x0_fn=None, correcting_xt_fn=None):
        if algorithm_type != "data_prediction":
            raise NotImplementedError("SASolver(algorithm_type=%r): only 'data_prediction', which the reference's sampler "
                                      "selects and recommends" % (algorithm_type,))
        if correcting_x0_fn is not None:
            raise NotImplementedError("SASolver(correcting_x0_fn=...): dynamic thresholding is not built")
        if correcting_xt_fn is not None:
            raise NotImplementedError("SASolver(correcting_xt_fn=...): no wrapper of the reference sets it")
        self.model = model
        self.condition, self.uncondition = condition, uncondition
        self.cfg_scale = float(cfg_scale)
        self.model_kwargs = dict(model_kwargs or {})
        alphas_cumprod = torch.from_numpy(np.cumprod(1.0 - linear_betas(diffusion_steps), axis=0)).to(torch.float32)
        self.ns = NoiseScheduleVP.from_alphas_cumprod(alphas_cumprod)
        self.predict_x0 = True
        self.sigma_min = float(self.ns.edm_sigma(torch.tensor([1e-3])))          # :357-358
        self.sigma_max = float(self.ns.edm_sigma(torch.tensor([1.0])))
        self._c2 = None
        self.model_input_dtype = torch.float32            # fused route: dtype of the latent handed to the model (it casts)
        self._tables = {}                                 # fused route: device coefficient tables by configuration

    # ---- data_prediction_fn (:377-386): one-element fp32 sigma_t / alpha_t, so an fp16 noise gives an fp32 x0
    def _x0_of_noise(self, x, t, noise):
        t = t.reshape(1)
        alpha_t, sigma_t = self.ns.marginal_alpha(t), self.ns.marginal_std(t)
        return (x - _on(sigma_t, x) * noise) / _on(alpha_t, x)

    def model_fn(self, x, t):
        return self._x0_of_noise(x, t, self._noise(x, t))

    # ---- get_time_steps (:398-418): N + 1 fp32 host times
    def get_time_steps(self, skip_type, t_T, t_0, N, order=1, device=None):
        if skip_type == "logSNR":
            lambda_T = self.ns.marginal_lambda(torch.tensor(t_T).reshape(1))
            lambda_0 = self.ns.marginal_lambda(torch.tensor(t_0).reshape(1))
            logSNR_steps = lambda_T + torch.linspace(torch.tensor(0.).item(), (lambda_0 - lambda_T).item() ** (1. / order),
                                                     N + 1).pow(order)
            return self.ns.inverse_lambda(logSNR_steps)
        if skip_type == "time":
            return torch.linspace(t_T ** (1. / order), t_0 ** (1. / order), N + 1).pow(order)
        if skip_type == "karras":
            sigma_min = max(0.002, self.sigma_min)
            sigma_max = min(80, self.sigma_max)
            sigma_steps = torch.linspace(sigma_max ** (1. / 7), sigma_min ** (1. / 7), N + 1).pow(7)
            return self.ns.edm_inverse_sigma(sigma_steps)
        raise ValueError("Unsupported skip_type %r, need to be 'logSNR' or 'time' or 'karras'" % (skip_type,))

    # ---- coefficients (:426-560).  s / e: interval start / end on the half-logSNR axis
    def get_coefficients_exponential_negative(self, order, s, e):
        """Integral of exp(-x) x^order over [s, e] (:426-447; the noise-prediction form, kept for completeness)."""
        assert order in [0, 1, 2, 3], "order is only supported for 0, 1, 2 and 3"
        if order == 0:
            return torch.exp(-e) * (torch.exp(e - s) - 1)
        if order == 1:
            return torch.exp(-e) * ((s + 1) * torch.exp(e - s) - (e + 1))
        if order == 2:
            return torch.exp(-e) * ((s ** 2 + 2 * s + 2) * torch.exp(e - s) - (e ** 2 + 2 * e + 2))
        return torch.exp(-e) * ((s ** 3 + 3 * s ** 2 + 6 * s + 6) * torch.exp(e - s) - (e ** 3 + 3 * e ** 2 + 6 * e + 6))

    def get_coefficients_exponential_positive(self, order, s, e, tau):
        """Integral of exp(x (1 + tau^2)) x^order over [s, e] (:449-476)."""
        assert order in [0, 1, 2, 3], "order is only supported for 0, 1, 2 and 3"
        ec = (1 + tau ** 2) * e                       # after the change of variable
        sc = (1 + tau ** 2) * s
        if order == 0:
            return torch.exp(ec) * (1 - torch.exp(-(ec - sc))) / ((1 + tau ** 2))
        if order == 1:
            return torch.exp(ec) * ((ec - 1) - (sc - 1) * torch.exp(-(ec - sc))) / ((1 + tau ** 2) ** 2)
        if order == 2:
            return torch.exp(ec) * ((ec ** 2 - 2 * ec + 2) - (sc ** 2 - 2 * sc + 2) * torch.exp(-(ec - sc))) / (
                (1 + tau ** 2) ** 3)
        return torch.exp(ec) * ((ec ** 3 - 3 * ec ** 2 + 6 * ec - 6) - (sc ** 3 - 3 * sc ** 2 + 6 * sc - 6) * torch.exp(
            -(ec - sc))) / ((1 + tau ** 2) ** 4)

    def lagrange_polynomial_coefficient(self, order, lambda_list):
        """Monomial coefficients of the Lagrange basis polynomials through lambda_list (:478-539)."""
        assert order in [0, 1, 2, 3]
        assert order == len(lambda_list) - 1
        L = lambda_list
        if order == 0:
            return [[1]]
        if order == 1:
            return [[1 / (L[0] - L[1]), -L[1] / (L[0] - L[1])],
                    [1 / (L[1] - L[0]), -L[0] / (L[1] - L[0])]]
        if order == 2:
            d1 = (L[0] - L[1]) * (L[0] - L[2])
            d2 = (L[1] - L[0]) * (L[1] - L[2])
            d3 = (L[2] - L[0]) * (L[2] - L[1])
            return [[1 / d1, (-L[1] - L[2]) / d1, L[1] * L[2] / d1],
                    [1 / d2, (-L[0] - L[2]) / d2, L[0] * L[2] / d2],
                    [1 / d3, (-L[0] - L[1]) / d3, L[0] * L[1] / d3]]
        d1 = (L[0] - L[1]) * (L[0] - L[2]) * (L[0] - L[3])
        d2 = (L[1] - L[0]) * (L[1] - L[2]) * (L[1] - L[3])
        d3 = (L[2] - L[0]) * (L[2] - L[1]) * (L[2] - L[3])
        d4 = (L[3] - L[0]) * (L[3] - L[1]) * (L[3] - L[2])
        return [[1 / d1, (-L[1] - L[2] - L[3]) / d1, (L[1] * L[2] + L[1] * L[3] + L[2] * L[3]) / d1,
                 (-L[1] * L[2] * L[3]) / d1],
                [1 / d2, (-L[0] - L[2] - L[3]) / d2, (L[0] * L[2] + L[0] * L[3] + L[2] * L[3]) / d2,
                 (-L[0] * L[2] * L[3]) / d2],
                [1 / d3, (-L[0] - L[1] - L[3]) / d3, (L[0] * L[1] + L[0] * L[3] + L[1] * L[3]) / d3,
                 (-L[0] * L[1] * L[3]) / d3],
                [1 / d4, (-L[0] - L[1] - L[2]) / d4, (L[0] * L[1] + L[0] * L[2] + L[1] * L[2]) / d4,
                 (-L[0] * L[1] * L[2]) / d4]]

    def get_coefficients_fn(self, order, interval_start, interval_end, lambda_list, tau):
        """The coefficients of the gradient terms (:541-560), data prediction."""
        assert order in [1, 2, 3, 4]
        assert order == len(lambda_list), "the length of lambda list must be equal to the order"
        lagrange = self.lagrange_polynomial_coefficient(order - 1, lambda_list)
        coefficients = []
        for i in range(order):
            coefficient = 0
            for j in range(order):
                coefficient += lagrange[i][j] * self.get_coefficients_exponential_positive(
                    order - 1 - j, interval_start, interval_end, tau)
            coefficients.append(coefficient)
        return coefficients

    # ---- the four updates (:562-753).  Their scalars come from ONE function, which the eager expression below and the
    # coefficient table of the fused step (pec_rows) both read
    def _update_scalars(self, corrector, few_steps, order, tau, t_prev_list, t):
        """(cx, [cg_0 .. cg_{order-1}], cn): x_t = cx * x + sum_i cg_i * model_prev_list[-(i + 1)] + cn * noise, each a
        one-element fp32 host tensor formed as the reference forms it before it meets a tensor:
        cx = exp(-tau^2 h) * (sigma_t / sigma_prev); cg_i = ((1 + tau^2) * sigma_t) * exp(-tau^2 lambda_t) * gc_i, gc the
        coefficients of get_coefficients_fn over [lambda_prev, lambda_t] - the predictor (Adams-Bashforth) interpolates
        through the previous times, the corrector (Adams-Moulton) through those and t - with the order-2 modification of
        the 'few steps' forms (:666-679, :723-734); cn = sigma_t * sqrt(1 - exp(-2 tau^2 h))."""
        assert order in [1, 2, 3, 4], "order of stochastic adams method is only supported for 1, 2, 3 and 4"
        ns = self.ns
        t = t.reshape(1)
        t_prev_list = [p.reshape(1) for p in t_prev_list]
        sigma_t = ns.marginal_std(t)
        lambda_t = ns.marginal_lambda(t)
        sigma_prev = ns.marginal_std(t_prev_list[-1])
        lambda_prev = ns.marginal_lambda(t_prev_list[-1])
        h = lambda_t - lambda_prev
        t_list = t_prev_list + [t] if corrector else t_prev_list
        lambda_list = [ns.marginal_lambda(t_list[-(i + 1)]) for i in range(order)]
        gc = self.get_coefficients_fn(order, lambda_prev, lambda_t, lambda_list, tau)
        if few_steps and order == 2:
            if corrector:
                mod = 1.0 * torch.exp((1 + tau ** 2) * lambda_t) * (
                    h / 2 - (h * (1 + tau ** 2) - 1 + torch.exp((1 + tau ** 2) * (-h))) / ((1 + tau ** 2) ** 2 * h))
            else:
                mod = 1.0 * torch.exp((1 + tau ** 2) * lambda_t) * (
                    h ** 2 / 2 - (h * (1 + tau ** 2) - 1 + torch.exp((1 + tau ** 2) * (-h))) / ((1 + tau ** 2) ** 2)) / (
                    lambda_prev - ns.marginal_lambda(t_prev_list[-2]))
            gc[0] = gc[0] + mod
            gc[1] = gc[1] - mod
        cg = [(1 + tau ** 2) * sigma_t * torch.exp(- tau ** 2 * lambda_t) * gc[i] for i in range(order)]
        cn = sigma_t * torch.sqrt(1 - torch.exp(-2 * tau ** 2 * h))
        cx = torch.exp(-tau ** 2 * h) * (sigma_t / sigma_prev)
        return cx, cg, cn

    def _update(self, corrector, few_steps, order, x, tau, model_prev_list, t_prev_list, noise, t):
        cx, cg, cn = self._update_scalars(corrector, few_steps, order, tau, t_prev_list, t)
        gradient_part = torch.zeros_like(x)
        for i in range(order):
            gradient_part += _on(cg[i], x) * model_prev_list[-(i + 1)]
        noise_part = _on(cn, x) * noise
        return _on(cx, x) * x + gradient_part + noise_part

    def adams_bashforth_update(self, order, x, tau, model_prev_list, t_prev_list, noise, t):
        """SA-Predictor (:562-600)."""
        return self._update(False, False, order, x, tau, model_prev_list, t_prev_list, noise, t)

    def adams_moulton_update(self, order, x, tau, model_prev_list, t_prev_list, noise, t):
        """SA-Corrector (:602-642)."""
        return self._update(True, False, order, x, tau, model_prev_list, t_prev_list, noise, t)

    def adams_bashforth_update_few_steps(self, order, x, tau, model_prev_list, t_prev_list, noise, t):
        """SA-Predictor with the order-2 modification (:644-698)."""
        return self._update(False, True, order, x, tau, model_prev_list, t_prev_list, noise, t)

    def adams_moulton_update_few_steps(self, order, x, tau, model_prev_list, t_prev_list, noise, t):
        """SA-Corrector with the order-2 modification (:700-753)."""
        return self._update(True, True, order, x, tau, model_prev_list, t_prev_list, noise, t)

    # ---- the loops (:755-1092)
    @staticmethod
    def orders_used(step, steps, predictor_order, corrector_order):
        """(predictor, corrector) order of loop step ``step`` = 1 .. steps: the warm-up (:807-808), then
        ``lower_order_final`` (:842-844)."""
        if step < max(predictor_order, corrector_order - 1):
            return min(predictor_order, step), min(corrector_order, step + 1)
        return min(predictor_order, steps - step + 1), min(corrector_order, steps - step + 2)

    @staticmethod
    def _draw(x, noise_steps, generator, i, out=None):
        """Draw number i of the loop's RNG stream (0: the one made before the first model call and never used), into
        ``out`` when given (the same stream: ``randn_like`` is ``normal_`` on a fresh tensor of that size)."""
        if noise_steps is not None:
            return noise_steps[i] if out is None else out.copy_(noise_steps[i])
        if out is not None:
            return out.normal_(generator=generator)
        if generator is None:
            return torch.randn_like(x)
        return torch.randn(x.shape, generator=generator, device=x.device, dtype=x.dtype)

    def _sample(self, few_steps, x, tau, steps, t_start, t_end, skip_type, skip_order, predictor_order, corrector_order,
                pc_mode, return_intermediate, noise_steps, generator, eps0):
        """sample_few_steps (:755-909: no corrector and tau = 0 on the last step, no model call after it) /
        sample_more_steps (:911-1064: corrector on the last step, then denoise to zero).  ``eps0``: the first model
        output when the fused route handed it back."""
        skip_final_step, denoise_to_zero = few_steps, not few_steps
        assert pc_mode in ["PEC", "PECE"], "Predictor-corrector mode only supports PEC and PECE"
        t_0 = 1. / self.ns.total_N if t_end is None else t_end
        t_T = self.ns.T if t_start is None else t_start
        assert t_0 > 0 and t_T > 0
        assert steps >= max(predictor_order, corrector_order - 1)
        timesteps = self.get_time_steps(skip_type, t_T, t_0, steps, skip_order)
        assert timesteps.shape[0] - 1 == steps
        bashforth = self.adams_bashforth_update_few_steps if few_steps else self.adams_bashforth_update
        moulton = self.adams_moulton_update_few_steps if few_steps else self.adams_moulton_update
        intermediates = []
        t = timesteps[0]
        if eps0 is None:
            self._draw(x, noise_steps, generator, 0)
            model_prev_list = [self.model_fn(x, t)]
        else:
            model_prev_list = [self._x0_of_noise(x, t, self._guide(eps0))]
        t_prev_list = [t]
        if return_intermediate:
            intermediates.append(x)
        warm = max(predictor_order, corrector_order - 1)
        for step in range(1, steps + 1):
            p_used, c_used = self.orders_used(step, steps, predictor_order, corrector_order)
            t = timesteps[step]
            noise = self._draw(x, noise_steps, generator, step)
            last = skip_final_step and step == steps
            x_p = bashforth(p_used, x, 0 if last else tau(t), model_prev_list, t_prev_list, noise, t)
            if not last:
                model_prev_list.append(self.model_fn(x_p, t))
            if corrector_order > 0 and not last:
                x = moulton(c_used, x, tau(t), model_prev_list, t_prev_list, noise, t)
                if pc_mode == "PECE" and step < steps:
                    model_prev_list[-1] = self.model_fn(x, t)
            else:
                x = x_p
            if return_intermediate:
                intermediates.append(x)
            t_prev_list.append(t)
            if step >= warm:
                del model_prev_list[0]
        if denoise_to_zero:
            x = self.model_fn(x, torch.ones((1,)) * t_0)
            if return_intermediate:
                intermediates.append(x)
        return (x, intermediates) if return_intermediate else x

    def sample_few_steps(self, x, tau, steps=5, t_start=None, t_end=None, skip_type="time", skip_order=1, predictor_order=3,
                         corrector_order=4, pc_mode="PEC", return_intermediate=False, noise_steps=None, generator=None):
        with torch.no_grad():
            return self._sample(True, x, tau, steps, t_start, t_end, skip_type, skip_order, predictor_order, corrector_order,
                                pc_mode, return_intermediate, noise_steps, generator, None)

    def sample_more_steps(self, x, tau, steps=20, t_start=None, t_end=None, skip_type="time", skip_order=1,
                          predictor_order=3, corrector_order=4, pc_mode="PEC", return_intermediate=False, noise_steps=None,
                          generator=None):
        with torch.no_grad():
            return self._sample(False, x, tau, steps, t_start, t_end, skip_type, skip_order, predictor_order,
                                corrector_order, pc_mode, return_intermediate, noise_steps, generator, None)

    # ---- the fused step (ops.cfg_sa_step): one launch per model call of the 'few_steps' PEC loop
    def pec_rows(self, tau, steps, t_start=None, t_end=None, skip_type="time", skip_order=1, predictor_order=2,
                 corrector_order=2):
        """The coefficient table of the fused step: [steps, SA_ROW] fp32 (host), row k for model call k at time ts[k]: x0
        of that call, the corrector of loop step k (none on row 0) and the predictor of loop step k + 1 - on the last row
        the final, predictor-only step with tau = 0 (layout: include/viditq.h, VQ_SA_*).  Every scalar is the one the eager
        update uses (_update_scalars, _t_val)."""
        from .. import _lib as L
        t_0 = 1. / self.ns.total_N if t_end is None else t_end
        t_T = self.ns.T if t_start is None else t_start
        assert steps >= max(predictor_order, corrector_order - 1)
        ts = self.get_time_steps(skip_type, t_T, t_0, steps, skip_order)
        rows = np.zeros((steps, L.SA_ROW), dtype=np.float32)
        for k in range(steps):
            r, t = rows[k], ts[k].reshape(1)
            r[L.SA_CFG] = self.cfg_scale
            r[L.SA_SIGMA], r[L.SA_ALPHA] = float(self.ns.marginal_std(t)), float(self.ns.marginal_alpha(t))
            prev = [ts[j] for j in range(max(k - 1, 0), k + 1)]           # t_prev_list[-2:] once step k is done
            if k > 0:
                oc = self.orders_used(k, steps, predictor_order, corrector_order)[1]
                assert oc in (1, 2), "the fused step serves corrector orders 1 and 2"
                cx, cg, cn = self._update_scalars(True, True, oc, tau(ts[k]), prev[:-1], ts[k])
                r[L.SA_OC], r[L.SA_CX], r[L.SA_CG0], r[L.SA_CN] = oc, float(cx), float(cg[0]), float(cn)
                if oc == 2:
                    r[L.SA_CG1] = float(cg[1])
            op = self.orders_used(k + 1, steps, predictor_order, corrector_order)[0]
            assert op in (1, 2), "the fused step serves predictor orders 1 and 2"
            cx, cg, cn = self._update_scalars(False, True, op, 0 if k + 1 == steps else tau(ts[k + 1]), prev, ts[k + 1])
            r[L.SA_OP], r[L.SA_PX], r[L.SA_PG0], r[L.SA_PN] = op, float(cx), float(cg[0]), float(cn)
            if op == 2:
                r[L.SA_PG1] = float(cg[1])
            r[L.SA_T_NEXT] = self._t_val(ts[k + 1])
        return torch.from_numpy(rows)

    def _fused_wanted(self, x, mode, pc_mode, predictor_order, corrector_order, steps, fused):
        if fused is None:
            fused = _SA_FUSED
        return (bool(fused) and mode == "few_steps" and pc_mode == "PEC" and 1 <= predictor_order <= 2
                and 1 <= corrector_order <= 2 and steps >= 2 and self.cfg_scale != 1.0 and self.uncondition is not None
                and x.is_cuda)

    def _pec_fused(self, x, tau, args, return_intermediate, noise_steps, generator):
        """The PEC loop with one launch behind each model call (fused_loop).  ``args``: the arguments of pec_rows behind
        tau, which with tau's values, the guidance scale, the device and n name the device table.  Returns (x,
        intermediates, None), or (None, None, eps) when the first model output is not one the kernel takes
        (ops.cfg_sa_step_ok): the caller goes on eagerly from it."""
        from .. import ops
        from .fused_loop import device_table, fused_loop
        n, steps = x.shape[0], args[0]
        x = x.float().contiguous() if x.dtype != torch.float32 or not x.is_contiguous() else x
        xm = torch.cat([x, x]).to(self.model_input_dtype)
        hist = torch.empty((2, x.numel()), dtype=torch.float32, device=x.device)
        ring = torch.empty((2,) + tuple(x.shape), dtype=torch.float32, device=x.device)
        text = self._joint_text()
        ts = self.get_time_steps(args[3], self.ns.T if args[1] is None else args[1],
                                 1. / self.ns.total_N if args[2] is None else args[2], steps, args[4])
        t = torch.full((2 * n,), self._t_val(ts[0]), dtype=torch.float32, device=x.device)
        taus = tuple(float(tau(v)) for v in ts)
        self._draw(x, noise_steps, generator, 0)
        state = dict(xp=x, mid=[x])

        def table(eps, x):
            if not ops.cfg_sa_step_ok(eps, x):
                return None
            return device_table(self._tables, (args, taus, self.cfg_scale, str(x.device), n),
                                lambda: self.pec_rows(tau, *args), x.device, n)

        def step(k, eps, x, rows):
            # the draw of loop step k + 1, from the eager route's RNG stream, into the slot the predictor reads
            self._draw(x, noise_steps, generator, k + 1, out=ring[(k + 1) % 2])
            # a fresh x_out where the intermediates are kept: what was handed out is never written again
            x, state["xp"] = ops.cfg_sa_step(eps, x, state["xp"], hist, ring, rows, k,
                                             x_out=None if return_intermediate or k == 0 else x,
                                             xp_out=None if k == 0 else state["xp"], x_model=xm)
            if k > 0:
                state["mid"].append(x)
            return x

        x_c, eps0 = fused_loop(steps, x, xm, t, lambda xm, t: self.model(xm, t, text, **self.model_kwargs), table, step)
        if x_c is None:
            return None, None, eps0
        return state["xp"], state["mid"] + [state["xp"]], None

    def step_graph(self, x, tau, steps, t_start=None, t_end=None, skip_type="time", skip_order=1, predictor_order=2,
                   corrector_order=2):
        """The counter form of the fused PEC loop: {model call, fused step, counter advance} captured once as a HIP graph
        and replayed ``steps`` times (graph.SAStepGraph); ``.run(x)`` samples."""
        from ..graph import SAStepGraph
        assert self.cfg_scale != 1.0 and self.uncondition is not None, "the fused step is the guided one"
        rows = self.pec_rows(tau, steps, t_start, t_end, skip_type, skip_order, predictor_order, corrector_order)
        t_T = self.ns.T if t_start is None else t_start
        t_0 = 1. / self.ns.total_N if t_end is None else t_end
        ts = self.get_time_steps(skip_type, t_T, t_0, steps, skip_order)
        return SAStepGraph(self.model, self._joint_text(), self.model_kwargs, x, rows, self._t_val(ts[0]),
                           self.model_input_dtype)

    @torch.no_grad()
    def sample(self, mode, x, tau, steps, t_start=None, t_end=None, skip_type="time", skip_order=1, predictor_order=3,
               corrector_order=4, pc_mode="PEC", return_intermediate=False, noise_steps=None, generator=None, fused=None):
        """``SASolver.sample`` (:1066-1092).  ``tau``: a callable of the (host, fp32) time.  ``noise_steps``: a pre-drawn
        [1 + steps, ...] stack used in place of the loop's draws (entry 0 is the draw the reference makes before the first
        model call and never uses); ``generator``: drawn from instead of the global one.  ``fused``: the route of the module
        docstring (None: the VQ_SA_FUSED switch, off by default)."""
        assert mode in ["few_steps", "more_steps"], "mode must be either 'few_steps' or 'more_steps'"
        eps0 = None
        if self._fused_wanted(x, mode, pc_mode, predictor_order, corrector_order, steps, fused):
            x_f, mid, eps0 = self._pec_fused(x, tau, (steps, t_start, t_end, skip_type, skip_order, predictor_order,
                                                      corrector_order), return_intermediate, noise_steps, generator)
            if x_f is not None:
                return (x_f, mid) if return_intermediate else x_f
        return self._sample(mode == "few_steps", x, tau, steps, t_start, t_end, skip_type, skip_order, predictor_order,
                            corrector_order, pc_mode, return_intermediate, noise_steps, generator, eps0)


class SASolverSampler:
    """Same call surface as t2i/diffusion/sa_sampler.py:10-94."""

    def __init__(self, model, noise_schedule="linear", diffusion_steps=1000, device="cpu"):
        if noise_schedule != "linear":
            raise NotImplementedError("SASolverSampler(noise_schedule=%r): only the linear betas of the released models"
                                      % (noise_schedule,))
        self.model, self.device, self.diffusion_steps = model, device, diffusion_steps
        self.model_input_dtype = torch.float32
        self._solver = None

    def solver(self, conditioning, unconditional_conditioning, unconditional_guidance_scale, model_kwargs) -> SASolver:
        """The SASolver of sa_sampler.py:75-88, kept while the arguments stay the same (its device tables with it)."""
        key = (conditioning, unconditional_conditioning, float(unconditional_guidance_scale))
        hit = self._solver
        if hit is None or hit[0][0] is not key[0] or hit[0][1] is not key[1] or hit[0][2] != key[2]:
            self._solver = hit = (key, SASolver(self.model, conditioning, unconditional_conditioning,
                                                unconditional_guidance_scale, None, self.diffusion_steps))
        hit[1].model_kwargs = dict(model_kwargs or {})
        hit[1].model_input_dtype = self.model_input_dtype
        return hit[1]

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, model_kwargs=None, fused=None, noise_steps=None, generator=None, **kwargs):
        """:31-94: 'few_steps', skip_type 'time', predictor 2, corrector 2, PEC, tau_t = eta inside [0.2, 0.8] and 0
        outside.  Returns (x, None)."""
        C, H, W = shape
        img = torch.randn((batch_size, C, H, W), device=self.device, generator=generator) if x_T is None else x_T
        solver = self.solver(conditioning, unconditional_conditioning, unconditional_guidance_scale, model_kwargs)
        tau_t = lambda t: eta if 0.2 <= t <= 0.8 else 0   # noqa: E731
        x = solver.sample(mode="few_steps", x=img, tau=tau_t, steps=S, skip_type="time", skip_order=1, predictor_order=2,
                          corrector_order=2, pc_mode="PEC", return_intermediate=False, fused=fused, noise_steps=noise_steps,
                          generator=generator)
        return x.to(self.device), None
