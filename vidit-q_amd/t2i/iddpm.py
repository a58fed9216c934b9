"""IDDPM ancestral sampling of the t2i scripts: ``--sampling_algo iddpm`` (quant_txt2img.py:154-166).

Restates ``IDDPM(str(steps)).p_sample_loop(model.forward_with_cfg, z.shape, z, clip_denoised=False, model_kwargs=...)``:
the factory t2i/diffusion/iddpm.py, SpacedDiffusion (t2i/diffusion/model/respace.py:65-134) and the sampling half of
GaussianDiffusion (t2i/diffusion/model/gaussian_diffusion.py: derived arrays :171-227, q_posterior_mean_variance :258-278,
p_mean_variance :280-361, _predict_xstart_from_eps :363-368, p_sample :405-446, p_sample_loop :448-540) for what the
factory's defaults give: epsilon prediction with a learned-range variance on the linear betas.

The respaced schedule (space_timesteps, linear_betas, the beta respacing) is the one of t2v/iddpm.py; this module adds the
posterior arrays.  Two routes compute a step:

eager   the reference's torch expressions, on whatever device the tensors are on (also the CPU).
fused   one launch of ops.cfg_ddpm_step per model call for the kept first half of the duplicated batch: the tail of
        forward_with_cfg, p_mean_variance and p_sample (47 small launches and eight pageable _extract_into_tensor
        uploads per step on the eager route, profiles/ddpm_step/README.md).  Taken by ``p_sample_loop(fused=True)`` or under VQ_DDPM_FUSED=1 when the latent is
        an fp32 GPU tensor, ``model`` is the bound ``forward_with_cfg`` of a net of this package and ``model_kwargs``
        carries ``y`` and ``cfg_scale``; everything else stays eager.  ``p_sample_graph`` captures {forward, step,
        counter advance} once (graph.DDPMStepGraph).
"""
from __future__ import annotations

import numpy as np
import torch

from ..t2v.iddpm import IDDPM as _RespacedSchedule
from .dpm_solver import _switch
from .pixart import CFG_GUIDED_CHANNELS as GUIDED, _PixArtBase

_DDPM_FUSED = _switch("VQ_DDPM_FUSED", False)        # guidance + variance + posterior step in one launch


def _extract_into_tensor(arr, timesteps, broadcast_shape):
    """gaussian_diffusion.py:1029-1041."""
    res = torch.from_numpy(arr).to(device=timesteps.device)[timesteps].float()
    while len(res.shape) < len(broadcast_shape):
        res = res[..., None]
    return res + torch.zeros(broadcast_shape, device=timesteps.device)


class SpacedDiffusion:
    """``SpacedDiffusion(space_timesteps(...), betas, EPSILON, LEARNED_RANGE, ...)`` for sampling."""

    def __init__(self, timestep_respacing, diffusion_steps=1000):
        s = _RespacedSchedule(timestep_respacing=timestep_respacing, diffusion_steps=diffusion_steps)
        self.timestep_map = s.timestep_map
        self.original_num_steps = diffusion_steps
        self.num_timesteps = s.num_timesteps
        betas = self.betas = s.betas
        self.alphas_cumprod, self.alphas_cumprod_prev = s.alphas_cumprod, s.alphas_cumprod_prev
        self.sqrt_recip_alphas_cumprod = s.sqrt_recip_alphas_cumprod
        self.sqrt_recipm1_alphas_cumprod = s.sqrt_recipm1_alphas_cumprod
        # the posterior q(x_{t-1} | x_t, x_0) (gaussian_diffusion.py:213-227), float64
        self.posterior_variance = betas * (1.0 - self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_log_variance_clipped = np.log(
            np.append(self.posterior_variance[1], self.posterior_variance[1:])
        ) if len(self.posterior_variance) > 1 else np.array([])
        self.posterior_mean_coef1 = betas * np.sqrt(self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_mean_coef2 = (1.0 - self.alphas_cumprod_prev) * np.sqrt(1.0 - betas) / (1.0 - self.alphas_cumprod)
        self.log_betas = np.log(betas)
        self.model_input_dtype = torch.float32            # fused route: dtype of the latent handed to the model (it casts)
        self._maps = {}                                   # timestep_map as a tensor, by (device, dtype)
        self._tables = {}                                 # fused route: device coefficient tables by configuration

    # ------------------------------------------------------------------ the eager route: the reference's expressions
    def _map_timesteps(self, t):
        """_WrappedModel (respace.py:129-131)."""
        key = (str(t.device), t.dtype)
        m = self._maps.get(key)
        if m is None:
            m = self._maps[key] = torch.tensor(self.timestep_map, device=t.device, dtype=t.dtype)
        return m[t]

    @staticmethod
    def _refuse(denoised_fn, cond_fn):
        if denoised_fn is not None:
            raise NotImplementedError("denoised_fn: no script of the reference passes one")
        if cond_fn is not None:
            raise NotImplementedError("cond_fn (classifier guidance): no script of the reference passes one")

    def q_posterior_mean_variance(self, x_start, x_t, t):
        """:258-278."""
        posterior_mean = (
            _extract_into_tensor(self.posterior_mean_coef1, t, x_t.shape) * x_start
            + _extract_into_tensor(self.posterior_mean_coef2, t, x_t.shape) * x_t
        )
        return (posterior_mean, _extract_into_tensor(self.posterior_variance, t, x_t.shape),
                _extract_into_tensor(self.posterior_log_variance_clipped, t, x_t.shape))

    def _predict_xstart_from_eps(self, x_t, t, eps):
        """:363-368."""
        return (
            _extract_into_tensor(self.sqrt_recip_alphas_cumprod, t, x_t.shape) * x_t
            - _extract_into_tensor(self.sqrt_recipm1_alphas_cumprod, t, x_t.shape) * eps
        )

    def p_mean_variance(self, model, x, t, clip_denoised=True, denoised_fn=None, model_kwargs=None, model_output=None):
        """:280-361 behind SpacedDiffusion's timestep mapping.  ``model_output``: what ``model`` would return, when the
        caller already has it."""
        self._refuse(denoised_fn, None)
        if model_kwargs is None:
            model_kwargs = {}
        B, C = x.shape[:2]
        assert t.shape == (B,)
        if model_output is None:
            model_output = model(x, timestep=self._map_timesteps(t), **model_kwargs)
        if isinstance(model_output, tuple):
            model_output, extra = model_output
        else:
            extra = None
        assert model_output.shape == (B, C * 2, *x.shape[2:])
        model_output, model_var_values = torch.split(model_output, C, dim=1)
        min_log = _extract_into_tensor(self.posterior_log_variance_clipped, t, x.shape)
        max_log = _extract_into_tensor(self.log_betas, t, x.shape)
        frac = (model_var_values + 1) / 2                  # [-1, 1] for [min_var, max_var]
        model_log_variance = frac * max_log + (1 - frac) * min_log
        model_variance = torch.exp(model_log_variance)
        pred_xstart = self._predict_xstart_from_eps(x_t=x, t=t, eps=model_output)
        if clip_denoised:
            pred_xstart = pred_xstart.clamp(-1, 1)
        model_mean, _, _ = self.q_posterior_mean_variance(x_start=pred_xstart, x_t=x, t=t)
        return {"mean": model_mean, "variance": model_variance, "log_variance": model_log_variance,
                "pred_xstart": pred_xstart, "extra": extra}

    def p_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, noise=None,
                 generator=None, model_output=None):
        """:405-446.  ``noise``: the draw to use instead of ``randn_like(x)`` (``generator``: its generator)."""
        self._refuse(denoised_fn, cond_fn)
        out = self.p_mean_variance(model, x, t, clip_denoised=clip_denoised, model_kwargs=model_kwargs,
                                   model_output=model_output)
        if noise is None:
            noise = torch.randn_like(x) if generator is None else torch.randn(
                x.shape, generator=generator, device=x.device, dtype=x.dtype)
        nonzero_mask = (t != 0).float().view(-1, *([1] * (len(x.shape) - 1)))     # no noise when t == 0
        sample = out["mean"] + nonzero_mask * torch.exp(0.5 * out["log_variance"]) * noise
        return {"sample": sample, "pred_xstart": out["pred_xstart"]}

    def _steps(self, model, img, clip_denoised, model_kwargs, noise_steps, generator, first_output=None):
        for k, i in enumerate(range(self.num_timesteps)[::-1]):
            t = torch.full((img.shape[0],), i, dtype=torch.long, device=img.device)
            with torch.no_grad():
                out = self.p_sample(model, img, t, clip_denoised=clip_denoised, model_kwargs=model_kwargs,
                                    noise=None if noise_steps is None else noise_steps[k], generator=generator,
                                    model_output=first_output if k == 0 else None)
            yield i, out
            img = out["sample"]

    @staticmethod
    def _start(model, shape, noise, device, generator):
        assert isinstance(shape, (tuple, list))
        if noise is not None:
            return noise
        if device is None:
            device = next(getattr(model, "__self__", model).parameters()).device
        return torch.randn(*shape, device=device, generator=generator)

    def p_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                  model_kwargs=None, device=None, progress=False, noise_steps=None, generator=None):
        """:493-540 (eager): yields p_sample's dict for i = num_timesteps - 1 .. 0."""
        self._refuse(denoised_fn, cond_fn)
        img = self._start(model, shape, noise, device, generator)
        steps = self._steps(model, img, clip_denoised, model_kwargs, noise_steps, generator)
        if progress:
            try:
                from tqdm.auto import tqdm
                steps = tqdm(steps, total=self.num_timesteps)
            except ImportError:
                pass
        for _, out in steps:
            yield out

    def p_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                      model_kwargs=None, device=None, progress=False, fused=None, noise_steps=None, generator=None,
                      step_callback=None):
        """:448-491.  ``fused``: the route of the module docstring (None: the VQ_DDPM_FUSED switch, off by default).
        ``noise_steps``: a pre-drawn [steps, 2n, C, ...] stack used in loop order instead of one ``randn`` of the
        duplicated shape per step (the fused step reads its first half).  ``step_callback(i, sample, pred_xstart)``
        after every step: the eager route hands it the whole duplicated batch, whose first half is the kept one, the
        fused route the kept half.  The fused route returns ``cat([x, x])``: ``samples.chunk(2, dim=0)[0]`` is the
        kept half on either route."""
        self._refuse(denoised_fn, cond_fn)
        img = self._start(model, shape, noise, device, generator)
        first = None
        net = self._fused_net(model, img, model_kwargs, fused)
        if net is not None:
            x, first = self._loop_fused(net, img, clip_denoised, model_kwargs, noise_steps, generator, step_callback)
            if x is not None:
                return torch.cat([x, x])
            first = net.guide_cfg(first, model_kwargs["cfg_scale"])
        final = None
        for i, out in self._steps(model, img, clip_denoised, model_kwargs, noise_steps, generator, first):
            if step_callback is not None:
                step_callback(i, out["sample"], out["pred_xstart"])
            final = out
        return final["sample"]

    # ------------------------------------------------------------------ the fused route
    def step_rows(self, cfg_scale, clip_denoised):
        """The coefficient table of the fused step: [steps, DDPM_ROW] fp32 (host) in loop order - row k belongs to
        i = steps - 1 - k - with the fp32 casts ``_extract_into_tensor(...).float()`` makes (layout: include/viditq.h,
        VQ_DDPM_*).  T_NEXT = timestep_map[i - 1], the model-input time of the forward that follows; on the last row
        (i = 0) that index wraps to the first forward's time, so a counter that ran through the table starts over."""
        from .. import _lib as L
        steps = self.num_timesteps
        rows = np.zeros((steps, L.DDPM_ROW), dtype=np.float32)
        for k in range(steps):
            i, r = steps - 1 - k, rows[k]
            r[L.DDPM_CFG] = cfg_scale
            r[L.DDPM_A], r[L.DDPM_B] = self.sqrt_recip_alphas_cumprod[i], self.sqrt_recipm1_alphas_cumprod[i]
            r[L.DDPM_C1], r[L.DDPM_C2] = self.posterior_mean_coef1[i], self.posterior_mean_coef2[i]
            r[L.DDPM_MIN_LOG], r[L.DDPM_MAX_LOG] = self.posterior_log_variance_clipped[i], self.log_betas[i]
            r[L.DDPM_NONZERO], r[L.DDPM_CLIP] = float(i != 0), float(bool(clip_denoised))
            r[L.DDPM_T_NEXT] = self.timestep_map[i - 1]
        return torch.from_numpy(rows)

    def _fused_net(self, model, img, model_kwargs, fused):
        """The net whose ``forward`` the fused route calls, or None for the eager route."""
        if fused is None:
            fused = _DDPM_FUSED
        net = getattr(model, "__self__", None)
        if not (fused and img.is_cuda and img.dtype == torch.float32 and img.shape[0] % 2 == 0 and img.dim() >= 3
                and isinstance(net, _PixArtBase)
                and getattr(model, "__func__", None) is _PixArtBase.forward_with_cfg
                and model_kwargs is not None and "y" in model_kwargs and "cfg_scale" in model_kwargs
                and self.num_timesteps > 1):
            return None
        return net

    @staticmethod
    def _split_kwargs(model_kwargs):
        kw = dict(model_kwargs)
        return kw.pop("y"), kw.pop("cfg_scale"), kw.pop("mask", None), kw

    @torch.no_grad()
    def _loop_fused(self, net, img, clip_denoised, model_kwargs, noise_steps, generator, step_callback):
        """The loop with one launch behind each model call (fused_loop).  Returns (x, None), or (None, model output) when
        the first model output is not one the kernel takes (ops.cfg_ddpm_step_ok): the caller goes on eagerly from it."""
        from .. import ops
        from .fused_loop import device_table, fused_loop
        n = img.shape[0] // 2
        y, cfg_scale, mask, kw = self._split_kwargs(model_kwargs)
        x = img[:n].contiguous()
        xm = torch.cat([x, x]).to(self.model_input_dtype)
        # the model-input time as fp32, which the counter form writes on the device; the nets cast it to their own dtype,
        # as they cast the reference's int64
        t = torch.full((2 * n,), float(self.timestep_map[-1]), dtype=torch.float32, device=x.device)

        def table(eps, x):
            if not ops.cfg_ddpm_step_ok(eps, x):
                return None
            return device_table(self._tables, (float(cfg_scale), bool(clip_denoised), str(x.device), n),
                                lambda: self.step_rows(cfg_scale, clip_denoised), x.device, n)

        def step(k, eps, x, rows):
            # the draw of the duplicated shape, as randn_like(x) of the reference: the RNG stream is the eager route's
            z = noise_steps[k] if noise_steps is not None else torch.randn(
                img.shape, generator=generator, device=x.device, dtype=torch.float32)
            x0 = torch.empty_like(x) if step_callback is not None else None
            # a fresh x_out per step: what a step_callback was handed is never written again
            x = ops.cfg_ddpm_step(eps, x, z[:n], rows, k, x0_out=x0, x_model=xm, guided=GUIDED)
            if step_callback is not None:
                step_callback(self.num_timesteps - 1 - k, x, x0)
            return x

        return fused_loop(self.num_timesteps, x, xm, t, lambda xm, t: net.forward(xm, t, y, mask, **kw), table, step)

    def p_sample_graph(self, model, noise, clip_denoised=True, model_kwargs=None):
        """The counter form of the fused loop: {forward, fused step, counter advance} captured once as a HIP graph and
        replayed ``num_timesteps`` times (graph.DDPMStepGraph); ``.run(z)`` samples.  ``noise``: the duplicated start
        latent [2n, C, ...] the buffers are shaped after."""
        from .._lib import VQError
        from ..graph import DDPMStepGraph
        net = self._fused_net(model, noise, model_kwargs, True)
        if net is None:
            raise VQError("p_sample_graph: the fused route needs an fp32 GPU latent, the bound forward_with_cfg of a net of "
                          "this package, and model_kwargs with y and cfg_scale")
        y, cfg_scale, mask, kw = self._split_kwargs(model_kwargs)
        return DDPMStepGraph(net.forward, y, mask, kw, noise[: noise.shape[0] // 2],
                             self.step_rows(cfg_scale, clip_denoised), float(self.timestep_map[-1]),
                             self.model_input_dtype, guided=GUIDED)


def IDDPM(timestep_respacing, noise_schedule="linear", use_kl=False, sigma_small=False, predict_xstart=False,
          learn_sigma=True, pred_sigma=True, rescale_learned_sigmas=False, diffusion_steps=1000, snr=False,
          return_startx=False) -> SpacedDiffusion:
    """Same call surface as t2i/diffusion/iddpm.py:9-53.  Sampling with the defaults - epsilon prediction, learned-range
    variance, linear betas - is what exists; the training-side switches (``snr``, ``return_startx``) have no effect on it."""
    for name, bad, why in (
            ("noise_schedule", noise_schedule != "linear", "only the linear betas of the released models"),
            ("use_kl", use_kl, "a training loss; sampling does not read it, and no script sets it"),
            ("rescale_learned_sigmas", rescale_learned_sigmas, "a training loss; no script sets it"),
            ("predict_xstart", predict_xstart, "the released nets predict epsilon"),
            ("learn_sigma", not learn_sigma, "the fixed-variance samplers are not built: the released nets learn the range"),
            ("pred_sigma", not pred_sigma, "a model without variance channels is not what forward_with_cfg returns")):
        if bad:
            raise NotImplementedError("IDDPM(%s=...): %s" % (name, why))
    if timestep_respacing is None or timestep_respacing == "":
        timestep_respacing = [diffusion_steps]
    return SpacedDiffusion(timestep_respacing, diffusion_steps)
