"""IDDPM / DDIM sampling loop: the caller of the hot path.

Mirrors t2v/opensora/schedulers/iddpm/__init__.py (IDDPM.sample :53-132, forward_with_cfg
:135-184), respace.py (space_timesteps :7-56, SpacedDiffusion :59-111) and the pieces of
gaussian_diffusion.py the DDIM path touches (beta schedule :110-135, derived arrays :170-200,
p_mean_variance :252-335, ddim_sample :514-552, ddim_sample_loop_progressive :639-782).

What runs where: the schedule is float64 numpy on the host, as in the reference; per step the host
passes three float32 coefficients to ONE fused kernel (CFG on eps[:, :3] + PTQD division + the
eta=0 DDIM update, csrc/sampler.hip) instead of ~25 torch elementwise launches and the
numpy->tensor `_extract_into_tensor` copies.  Timesteps are known on the host, so the model is
called with ``timestep_id`` and the reference's per-forward ``t[0].item()`` sync disappears.

As-released behaviours kept: guidance on 3 of the 4 eps channels; the kept sample
is the first half of the duplicated batch; PTQD ``1/(1+k)`` with k looked up by (999-t)//50 -
``ks`` is an explicit optional argument here (default 0) because the reference's file
(./t2v/rebuttal_files/k_for_each_timestep.pth) is not shipped.

The fused route (``fused=True`` or VQ_T2V_DDIM_FUSED=1, off by default): per step ``forward(patch_major=True)`` once
(joint) or twice (``cfg_split``) and one ops.cfg_ddim_step_patch, which reads final_layer's output where the model left
it - no unpatchify copy, no fp32 cast, no ``torch.full`` / ``torch.cat`` on the host - takes its scalars (PTQD's 1 + k
among them) from a device table (``ddim_rows``) and writes the next forward's input in the model's dtype.  Bit-identical
to the eager expressions on the same device.  ``step_graph`` is its one-graph form (graph.VideoDDIMStepGraph).
"""
from __future__ import annotations

import inspect
import os
from typing import Optional

import numpy as np
import torch

from .. import _lib, ops

# the patch-major step behind each forward.  Read once, here (t2i imports this module: its _switch
# cannot be imported from here)
_T2V_DDIM_FUSED = os.environ.get("VQ_T2V_DDIM_FUSED", "0") != "0"


def get_key_for_value(dict_ranges, value):
    """gaussian_diffusion.py:24-29: first "hi-lo" key whose closed range holds ``value`` (keys are walked
    in file order; a non-range key such as ``fp_layers`` raises exactly as in the reference)."""
    for key in dict_ranges:
        range_start, range_end = map(int, key.split("-"))
        if range_start >= value >= range_end:
            return key
    return None


class TimestepMP:
    """Per-step mixed-precision switching of ddim_sample_loop_progressive (gaussian_diffusion.py:740-759).

    Driven by the attributes the reference script sets on the QuantModel (quant_txt2video_mp.py:373,
    533-540): ``timestep_wise_mp``, ``time_mp_config_weight`` (``{"hi-lo": {layer: bits}, ...,
    "fp_layers": {"hi-lo": [patterns]}}``) and ``time_mp_config_act``.  The key is looked up with the loop
    index i (position in the respaced schedule), not the raw timestep."""

    def __init__(self, qnn):
        self.qnn = qnn
        self.key_org = None
        self.fp_layer_list_org = None

    def apply(self, i: int):
        qnn = self.qnn
        key = get_key_for_value(qnn.time_mp_config_weight, i)
        if key is None:
            raise RuntimeError("this timestep %d is not included by the config" % i)
        if key != self.key_org:
            if self.fp_layer_list_org is not None:
                qnn.set_layer_quant(model=qnn, module_name_list=self.fp_layer_list_org, quant_level="per_layer",
                                    weight_quant=True, act_quant=True, prefix="")
            fp_layer_list = qnn.time_mp_config_weight["fp_layers"][key]
            qnn.set_layer_quant(model=qnn, module_name_list=fp_layer_list, quant_level="per_layer",
                                weight_quant=False, act_quant=False, prefix="")
            qnn.load_bitwidth_config(model=qnn, bit_config=qnn.time_mp_config_weight[key], bit_type="weight")
            qnn.load_bitwidth_config(model=qnn, bit_config=qnn.time_mp_config_act[key], bit_type="act")
            self.key_org = key
            self.fp_layer_list_org = fp_layer_list
        return key


def space_timesteps(num_timesteps, section_counts):
    """respace.py:7-56."""
    if isinstance(section_counts, str):
        if section_counts.startswith("ddim"):
            desired_count = int(section_counts[len("ddim"):])
            for i in range(1, num_timesteps):
                if len(range(0, num_timesteps, i)) == desired_count:
                    return set(range(0, num_timesteps, i))
            raise ValueError("cannot create exactly %d steps with an integer stride" % num_timesteps)
        section_counts = [int(x) for x in section_counts.split(",")]
    size_per = num_timesteps // len(section_counts)
    extra = num_timesteps % len(section_counts)
    start_idx = 0
    all_steps = []
    for i, section_count in enumerate(section_counts):
        size = size_per + (1 if i < extra else 0)
        if size < section_count:
            raise ValueError("cannot divide section of %d steps into %d" % (size, section_count))
        frac_stride = 1 if section_count <= 1 else (size - 1) / (section_count - 1)
        cur_idx = 0.0
        taken = []
        for _ in range(section_count):
            taken.append(start_idx + round(cur_idx))
            cur_idx += frac_stride
        all_steps += taken
        start_idx += size
    return set(all_steps)


def linear_betas(num_diffusion_timesteps=1000):
    """gaussian_diffusion.py:118-127."""
    scale = 1000 / num_diffusion_timesteps
    return np.linspace(scale * 0.0001, scale * 0.02, num_diffusion_timesteps, dtype=np.float64)


class IDDPM:
    """Spaced Gaussian diffusion with epsilon prediction and learned-range variance; DDIM sampler."""

    def __init__(self, num_sampling_steps=None, timestep_respacing=None, diffusion_steps=1000, cfg_scale=4.0):
        if num_sampling_steps is not None:
            assert timestep_respacing is None
            timestep_respacing = str(num_sampling_steps)
        if timestep_respacing is None or timestep_respacing == "":
            timestep_respacing = [diffusion_steps]
        base_betas = linear_betas(diffusion_steps)
        base_acp = np.cumprod(1.0 - base_betas, axis=0)
        use = space_timesteps(diffusion_steps, timestep_respacing)
        self.timestep_map = []
        last = 1.0
        new_betas = []
        for i, acp in enumerate(base_acp):       # respace.py:72-77
            if i in use:
                new_betas.append(1 - acp / last)
                last = acp
                self.timestep_map.append(i)
        betas = np.array(new_betas, dtype=np.float64)
        self.betas = betas
        self.num_timesteps = int(betas.shape[0])
        alphas = 1.0 - betas
        self.alphas_cumprod = np.cumprod(alphas, axis=0)
        self.alphas_cumprod_prev = np.append(1.0, self.alphas_cumprod[:-1])
        self.sqrt_recip_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod)
        self.sqrt_recipm1_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod - 1)
        self.cfg_scale = cfg_scale
        self._tables = {}                        # fused_loop.device_table: (cfg, ks, device, n) -> table on the device

    # ------------------------------------------------------------------ one DDIM step
    def ddim_step(self, x, cond_out, uncond_out, i: int, cfg_scale: float, k: float = 0.0, out=None):
        """x, x_next: fp32 [n, C, ...]; cond/uncond model outputs fp32 [n, 2C, ...]; eta = 0."""
        A = np.float32(self.sqrt_recip_alphas_cumprod[i])
        Bc = np.float32(self.sqrt_recipm1_alphas_cumprod[i])
        abp = np.float32(self.alphas_cumprod_prev[i])
        return ops.cfg_ddim_step(cond_out.contiguous(), uncond_out.contiguous(), x.contiguous(), cfg_scale, 1.0 + k,
                                 float(A), float(Bc), float(abp), out=out)

    def ddim_rows(self, cfg_scale: float, ks=None) -> torch.Tensor:
        """The coefficient table of ops.cfg_ddim_step_patch, fp32 [num_timesteps, DDIM_ROW] in LOOP order (row 0 is the
        first step, the highest t): per row the np.float32 scalars ``ddim_step`` passes for that step - cfg, 1 + k with
        ``ks`` looked up as in the loop, A, Bc, abar_prev - and, in the slot every row layout shares, the model-input
        time of the NEXT forward (the last row repeats its own)."""
        rows = np.zeros((self.num_timesteps, _lib.DDIM_ROW), dtype=np.float32)
        order = list(range(self.num_timesteps))[::-1]
        for r, i in enumerate(order):
            t_id = self.timestep_map[i]
            k = 0.0 if ks is None else float(ks[(999 - t_id) // 50])
            rows[r, _lib.DDIM_CFG] = np.float32(cfg_scale)
            rows[r, _lib.DDIM_ONE_PLUS_K] = np.float32(1.0 + k)
            rows[r, _lib.DDIM_A] = np.float32(self.sqrt_recip_alphas_cumprod[i])
            rows[r, _lib.DDIM_BC] = np.float32(self.sqrt_recipm1_alphas_cumprod[i])
            rows[r, _lib.DDIM_ABAR_PREV] = np.float32(self.alphas_cumprod_prev[i])
            rows[r, _lib.DDIM_T_NEXT] = np.float32(self.timestep_map[order[min(r + 1, len(order) - 1)]])
        return torch.from_numpy(rows)

    # ------------------------------------------------------------------ full loop
    @torch.no_grad()
    def sample(self, model, text_encoder, sampler_type, z_size, prompts, device, return_trajectory=False,
               additional_args=None, init_noise=None, ks: Optional[torch.Tensor] = None, generator=None,
               progress=False, fused=None):
        """iddpm/__init__.py:53-132.  Returns the n kept samples [n, *z_size] fp32.  ``fused``: ddim_sample_loop's."""
        if sampler_type != "ddim":
            raise NotImplementedError("only sampler_type='ddim' works in the reference (SURVEY A.4-5)")
        n = len(prompts)
        if init_noise is None:
            z = torch.randn(n, *z_size, device=device, generator=generator)
        else:
            z = init_noise.to(device)
        model_args = {}
        if additional_args is not None and "precompute_text_embeds" in additional_args:
            choose_idx = additional_args["batch_ids"]
            pre = additional_args["precompute_text_embeds"]
            ysel = pre["y"][choose_idx]                       # [n, 2, 1, L, Cc]
            sh = ysel.shape
            model_args["y"] = ysel.permute(1, 0, 2, 3, 4).reshape(n * sh[1], sh[2], sh[3], sh[4])
            model_args["mask"] = pre["mask"][choose_idx]
        else:
            enc = text_encoder.encode(prompts)
            model_args["y"] = torch.cat([enc["y"], text_encoder.null(n)], 0)
            if "mask" in enc:
                model_args["mask"] = enc["mask"]
        if additional_args is not None:
            for k_, v_ in additional_args.items():
                if k_ not in ("precompute_text_embeds", "batch_ids"):
                    model_args[k_] = v_
        return self.ddim_sample_loop(model, z, model_args, ks=ks, progress=progress, fused=fused)

    @torch.no_grad()
    def ddim_sample_loop(self, model, z, model_args, ks=None, progress=False, step_callback=None, graphed=False,
                         fused=None):
        """x: the kept half only (both halves evolve identically in the reference: :161-162).
        ``graphed``: replay the two forward-samples of a step from a HIP graph (one graph per smooth-quant
        time-range and mixed-precision key, graph.GraphedSampler); needs ``cfg_split`` and a QuantModel.
        ``fused``: the patch-major forwards and ops.cfg_ddim_step_patch per step (None reads the VQ_T2V_DDIM_FUSED
        switch); CPU tensors, a model whose forward takes no ``patch_major`` and a model output the entry point
        refuses run the eager expressions, the last from the forward already made."""
        x = z.float().contiguous()
        n = x.shape[0]
        y, mask = model_args["y"], model_args.get("mask")
        extra = {k: v for k, v in model_args.items() if k not in ("y", "mask")}
        cfg_split = bool(getattr(model, "cfg_split", False))
        y_cond, y_uncond = y[:n], y[n:]
        buf = torch.empty_like(x)
        indices = list(range(self.num_timesteps))[::-1]
        mp = TimestepMP(model) if getattr(model, "timestep_wise_mp", False) else None
        gs = None
        if graphed:
            from ..graph import GraphedSampler
            assert cfg_split and _accepts_timestep_id(model) and not extra, "graphed sampling: cfg_split QuantModel"
            gs = GraphedSampler(model, y_cond, y_uncond, mask)
        first = None
        if (_T2V_DDIM_FUSED if fused is None else fused) and gs is None and x.is_cuda and takes_patch_major(model):
            x_f, first = self._ddim_fused(model, x, y_cond, y_uncond, mask, extra, cfg_split, ks, mp, step_callback)
            if x_f is not None:
                return x_f
        for i in indices:
            t_id = self.timestep_map[i]
            key = mp.apply(i) if mp is not None else None
            if first is not None:                          # the refused output of the fused route: not computed again
                (cond, uncond), first = first, None
            elif gs is not None:
                cond, uncond = gs.forward_pair(x, t_id, key)
            else:
                t = torch.full((n,), t_id, device=x.device, dtype=torch.long)
                cond, uncond = model_forward_pair(model, x, t, y_cond, y_uncond, mask, cfg_split, t_id, extra)
            k = 0.0 if ks is None else float(ks[(999 - t_id) // 50])
            out = self.ddim_step(x, cond, uncond, i, self.cfg_scale, k, out=buf)
            x, buf = out, x
            if step_callback is not None:
                step_callback(i, x)
        return x

    def _ddim_fused(self, model, x, y_cond, y_uncond, mask, extra, cfg_split, ks, mp, step_callback):
        """The loop above with the patch-major forwards and step.  Returns (x, None), or (None, (cond, uncond)) - the first
        step's model outputs as the eager step takes them - when ops.cfg_ddim_step_patch_ok refuses them."""
        from ..t2i.fused_loop import device_table, fused_loop
        n = x.shape[0]
        copies = 1 if cfg_split else 2
        patch = tuple(model.patch_size)
        texts = (y_cond, y_uncond) if cfg_split else torch.cat([y_cond, y_uncond], 0)
        takes_id = _accepts_timestep_id(model)
        x = x.clone()                                      # the step writes in place; the caller's latent stays
        xm = torch.cat([x] * copies).to(getattr(model, "dtype", torch.float32))
        indices = list(range(self.num_timesteps))[::-1]
        t = torch.full((copies * n,), float(self.timestep_map[indices[0]]), dtype=torch.float32, device=x.device)

        def forward(xm, t):
            i = indices[call[0]]
            call[0] += 1
            if mp is not None:
                mp.apply(i)
            kw = dict(extra, mask=mask)
            if takes_id:
                kw["timestep_id"] = self.timestep_map[i]
            return patch_forward_pair(model, xm, t[:copies * n], texts, cfg_split, kw)

        def table(eps, x):
            if not ops.cfg_ddim_step_patch_ok(eps[0], eps[1], x, patch):
                return None
            key = (float(self.cfg_scale), None if ks is None else tuple(float(v) for v in ks), str(x.device), n)
            return device_table(self._tables, key, lambda: self.ddim_rows(self.cfg_scale, ks), x.device, n)

        def step(k, eps, x, rows):
            ops.cfg_ddim_step_patch(eps[0], eps[1], x, rows, k, patch, x_out=x, x_model=xm)
            if step_callback is not None:
                step_callback(indices[k], x)
            return x

        call = [0]
        x_f, eps0 = fused_loop(self.num_timesteps, x, xm, t, forward, table, step)
        if x_f is not None:
            return x_f, None
        return None, tuple(model.unpatchify(e).to(torch.float32) for e in eps0)

    def step_graph(self, model, x, model_args, ks=None, warmup=2):
        """The counter form of the fused loop: {forward(s), patch-major step, counter advance} captured as HIP graphs - one
        per smooth-quant time range the schedule visits - and replayed ``num_timesteps`` times; ``.run(x)`` samples from a
        start latent [n, ...].  PTQD's ``ks`` rides in the table."""
        from ..graph import VideoDDIMStepGraph
        return VideoDDIMStepGraph(self, model, x, model_args, ks=ks, warmup=warmup)


def takes_patch_major(model) -> bool:
    """Whether ``model.forward`` (a QuantModel's wrapped model's) has the ``patch_major`` argument of STDiT.forward."""
    target = getattr(model, "model", model) if _accepts_timestep_id(model) else model
    try:
        return "patch_major" in inspect.signature(target.forward).parameters
    except (TypeError, ValueError):
        return False


def patch_forward_pair(model, xm, t, texts, cfg_split, kw, side=None):
    """The patch-major forwards of one denoising step, (first, second) in the order of ``texts``.  Joint: ``texts`` is the
    joint text of 2n samples and the result the two halves of ONE forward of ``xm`` [2n, ...].  ``cfg_split``: ``texts``
    is a pair and each gets a forward of ``xm`` [n, ...], the first and then the second - the second's chain on the stream
    ``side`` when one is given (a capture forks it as graph.StepGraph does).  ``kw``: mask, timestep_id and the rest."""
    if not cfg_split:
        n = xm.shape[0] // 2
        out = model.forward(xm, t, texts, patch_major=True, **kw)
        return out[:n], out[n:]
    if side is None:
        first = model.forward(xm, t, texts[0], patch_major=True, **kw)
        return first, model.forward(xm, t, texts[1], patch_major=True, **kw)
    cur = torch.cuda.current_stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        second = model.forward(xm, t, texts[1], patch_major=True, **kw)
    first = model.forward(xm, t, texts[0], patch_major=True, **kw)
    cur.wait_stream(side)
    return first, second


def model_forward_pair(model, x, t, y_cond, y_uncond, mask, cfg_split, t_id, extra):
    """The two forward-samples of one denoising step (iddpm/__init__.py:141-163)."""
    kw = dict(extra)
    if _accepts_timestep_id(model):
        kw["timestep_id"] = t_id
    if cfg_split:
        cond = model.forward(x, t, y_cond, mask=mask, **kw)
        uncond = model.forward(x, t, y_uncond, mask=mask, **kw)
    else:
        n = x.shape[0]
        out = model.forward(torch.cat([x, x], 0), torch.cat([t, t], 0), torch.cat([y_cond, y_uncond], 0),
                            mask=mask, **kw)
        cond, uncond = out[:n], out[n:]
    return cond, uncond


def _accepts_timestep_id(model) -> bool:
    from ..qdiff.models.quant_model import QuantModel
    return isinstance(model, QuantModel)


def forward_with_cfg(model, x, timestep, y, cfg_scale, ks=None, **kwargs):
    """API-compatible restatement of iddpm/__init__.py:135-184 returning [2n, 2C, ...] like the
    reference (guided eps on channels 0-2, raw on the rest).  The sampling loop above does not call
    this; it exists for drop-in callers and for parity tests of the CFG rule."""
    n = len(x) // 2
    half = x[:n]
    cfg_split = bool(getattr(model, "cfg_split", False))
    if cfg_split:
        yc, yu = y[:n], y[n:]
        tc, tu = timestep[:n], timestep[n:]
        out = torch.cat([model.forward(half, tc, yc, **kwargs), model.forward(half, tu, yu, **kwargs)], dim=0)
    else:
        out = model.forward(torch.cat([half, half], dim=0), timestep, y, **kwargs)
    k = 0.0 if ks is None else float(ks[(999 - int(timestep[0])) // 50])
    out = out / (1 + k)
    eps, rest = out[:, :3], out[:, 3:]
    cond_eps, uncond_eps = torch.split(eps, n, dim=0)
    half_eps = uncond_eps + cfg_scale * (cond_eps - uncond_eps)
    return torch.cat([torch.cat([half_eps, half_eps], dim=0), rest], dim=1)
