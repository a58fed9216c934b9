"""HIP-graph capture of the per-step forwards.

One denoising step launches ~2300 kernels from Python (28 blocks x ~20 kernels x 2 forward-samples);
at ~64 ms of GPU work per step the eager loop is partly host-bound.  Shapes, buffers and the kernel
sequence are static within a smooth-quant time-range, so both forward-samples of a step (cond +
uncond) are captured ONCE into a HIP graph (``torch.cuda.CUDAGraph`` records the raw
``hipLaunchKernelGGL`` calls our C ABI makes on the capturing stream) and replayed with new latent /
timestep / text-embedding contents copied into the static input buffers.  One graph per time-range
(the packed weights and smoothing vectors differ between ranges) and per mixed-precision key (the
per-layer bit widths and FP layer set differ between keys, iddpm.TimestepMP).
"""
from __future__ import annotations

import os
from typing import Dict, Hashable, Optional, Tuple

import torch


def _capture(fn, warmup: int, first=None, debug: bool = False):
    """One call of ``fn`` recorded as a HIP graph.  Before the capture, on a side stream: ``first`` (when given, and waited
    for) and ``warmup`` calls of ``fn`` - they pack weights and fill the host-side caches (fused qkv weights, prompt K/V,
    mask selection) with the capture's own launch pattern.  ``debug``: the graph keeps what ``debug_dump`` needs.
    Returns (graph, what the recorded call returned)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        if first is not None:
            first()
            side.synchronize()
        for _ in range(warmup):
            fn()
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    if debug:
        graph.enable_debug_mode()
    # thread_local: with a process group alive (N > 1) the RCCL watchdog thread polls events while we capture; in
    # the default 'global' mode such a call from ANOTHER thread would invalidate the capture
    with torch.no_grad(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out = fn()
    return graph, out


class StepGraph:
    """cond/uncond forwards of a QuantModel for one prompt as a replayable HIP graph."""

    def __init__(self, qnn, x: torch.Tensor, y_cond: torch.Tensor, y_uncond: torch.Tensor,
                 mask: Optional[torch.Tensor], timestep_id: int, warmup: int = 2, two_streams: bool = True):
        self.qnn = qnn
        # cond and uncond are independent chains: captured as two parallel branches of the graph (fork /
        # join through a second HIP stream) so that the HBM-bound kernels of one chain (quantizers,
        # temporal attention: few VGPRs, no LDS) can run on CUs whose MFMA pipes the other chain's GEMM
        # workgroups keep busy
        self.two_streams = two_streams
        self.side = torch.cuda.Stream() if two_streams else None
        self.x = x.clone()
        self.t = torch.full((x.shape[0],), int(timestep_id), device=x.device, dtype=torch.long)
        self.yc, self.yu = y_cond.clone(), y_uncond.clone()
        self.mask = mask
        self.cfg_split = bool(getattr(qnn, "cfg_split", False))
        from . import _lib
        dump = os.environ.get("VQ_GRAPH_DUMP")          # measurement: a .dot file of the captured graph (node census, bench.py)

        def counted():
            # C-ABI calls of one step; the last call is the recorded one (= the graph's HIP-kernel nodes from this library:
            # one launch per entry point, the fast quantizer entry points included; the ~60 torch elementwise kernels of
            # the FP edges come on top)
            calls0 = _lib.CALLS[0]
            out = self._forward(timestep_id)
            self.c_abi_calls = _lib.CALLS[0] - calls0
            return out

        # first pass on ONE stream: it packs weights and fills the module-level caches.  Run on two streams that pass would
        # let the cond chain read a cached tensor that the uncond chain's stream is still producing - and such a tensor
        # would persist into the captured graph
        self.graph, (self.cond, self.uncond) = _capture(counted, warmup, debug=bool(dump),
                                                        first=lambda: self._forward(timestep_id, serial=True))
        self.dot_path = None
        if dump:
            try:
                self.dot_path = "%s.%d.dot" % (dump, id(self))
                self.graph.debug_dump(self.dot_path)
            except Exception:                           # the census is optional; the capture itself stands
                self.dot_path = None

    def _forward(self, t_id, serial=False):
        q = self.qnn
        if self.cfg_split and self.two_streams and not serial:
            cur = torch.cuda.current_stream()
            self.side.wait_stream(cur)
            with torch.cuda.stream(self.side):
                unc = q(self.x, self.t, self.yu, mask=self.mask, timestep_id=t_id)
            cond = q(self.x, self.t, self.yc, mask=self.mask, timestep_id=t_id)
            cur.wait_stream(self.side)
            return cond, unc
        if self.cfg_split:
            return (q(self.x, self.t, self.yc, mask=self.mask, timestep_id=t_id),
                    q(self.x, self.t, self.yu, mask=self.mask, timestep_id=t_id))
        n = self.x.shape[0]
        out = q(torch.cat([self.x, self.x]), torch.cat([self.t, self.t]), torch.cat([self.yc, self.yu]),
                mask=self.mask, timestep_id=t_id)
        return out[:n], out[n:]

    def run(self, x: torch.Tensor, timestep_id: int):
        self.x.copy_(x)
        self.t.fill_(int(timestep_id))
        self.graph.replay()
        return self.cond, self.uncond


class GraphedSampler:
    """Lazily captures one StepGraph per (smooth-quant time-range, mixed-precision key) of ``qnn``."""

    def __init__(self, qnn, y_cond, y_uncond, mask, two_streams: bool = True):
        self.qnn, self.yc, self.yu, self.mask = qnn, y_cond, y_uncond, mask
        self.two_streams = two_streams
        self.graphs: Dict[Tuple[int, Hashable], StepGraph] = {}
        self._epoch = None

    def _range_of(self, t_id: int) -> int:
        from .qdiff.models.quant_layer import find_interval
        for _, layer in self.qnn.quant_layers():
            if getattr(layer, "smooth_quant", False) and hasattr(layer, "timerange"):
                return find_interval(layer.timerange, t_id)
        return 0

    def forward_pair(self, x, t_id: int, mp_key: Hashable = None):
        """``mp_key``: whatever identifies the current per-layer bit-width / FP-layer state (the caller has
        already applied it to ``qnn``); a new key captures a new graph."""
        from .qdiff.models.quant_layer import PACK_EPOCH
        if self._epoch != PACK_EPOCH[0]:
            # some layer dropped its packed weights since the last capture (invalidate_packed / set_quant_params_dict):
            # the captured graphs reference the freed buffers - drop them, the next call captures afresh
            self.graphs.clear()
            self._epoch = PACK_EPOCH[0]
        r = (self._range_of(t_id), mp_key)
        g = self.graphs.get(r)
        if g is None:
            g = self.graphs[r] = StepGraph(self.qnn, x, self.yc, self.yu, self.mask, t_id,
                                           two_streams=self.two_streams)
        return g.run(x, t_id)


def _ident(v):
    """Identity of a keyword argument for the graph key: tensors by storage and version (their CONTENT is baked into the
    capture through host-side decisions such as the prompt-token selection), containers recursively, scalars by value."""
    if torch.is_tensor(v):
        return ("t", v.data_ptr(), v._version, tuple(v.shape), str(v.dtype))
    if isinstance(v, dict):
        return tuple((k, _ident(x)) for k, x in sorted(v.items()))
    if isinstance(v, (list, tuple)):
        return tuple(_ident(x) for x in v)
    return v


class ForwardGraph:
    """One forward ``fn(x, t, y, **kwargs)`` as a replayable HIP graph with static x / t / y buffers."""

    def __init__(self, fn, x, t, y, kwargs, warmup: int = 2):
        self.x, self.t, self.y = x.clone(), t.clone(), y.clone()
        self.kwargs = kwargs
        self.graph, self.out = _capture(lambda: fn(self.x, self.t, self.y, **kwargs), warmup + 1)

    def run(self, x, t, y):
        self.x.copy_(x)
        self.t.copy_(t)
        self.y.copy_(y)
        self.graph.replay()
        return self.out


class GraphedModel:
    """``model(x, t, y, **kwargs)`` for a sampling loop that calls one forward per step with the same shapes and the same
    keyword arguments (the t2i DPM-Solver loop, quant_txt2img.py:130-153: ``DPMS_sigma(GraphedModel(qnn.forward_with_dpmsolver),
    ...)``).  The ~540 launches of a PixArt forward are captured once per (shapes, keyword identities, smooth-quant
    time-range, per-layer quant state and bit widths, pack epoch) and replayed with the new latent / timestep / text embedding copied into the static inputs;
    the result is a fresh tensor each call (multistep solvers keep earlier outputs).  Bit-identical to eager launches
    (tested).  At PixArt-Sigma 1024 x 1024 a forward is 19.9 ms of GPU work either way (50.3 steps/s eager, 49.7
    replayed): eager Python launches need 10.9 ms of host time per step and stay ahead of the GPU, a replay needs 3.0 ms;
    the replay pays when the forward is shorter than its ~25 us per launch from Python (small latents) or the host
    is needed for something else."""

    def __init__(self, fn, qnn=None, max_graphs: int = 8):
        self.fn, self.qnn = fn, qnn if qnn is not None else getattr(fn, "__self__", None)
        self.graphs: Dict[Hashable, ForwardGraph] = {}
        self.max_graphs = max_graphs
        self._epoch = None
        self._qlayers = None

    def _layers(self):
        """The QuantLayers under the wrapped model, collected once (wrapping happens before the loop; the module tree
        does not change afterwards)."""
        if self._qlayers is None:
            root = self.qnn
            from .qdiff.models.quant_layer import QuantLayer
            self._qlayers = [m for m in root.modules() if isinstance(m, QuantLayer)] \
                if root is not None and hasattr(root, "modules") else []
        return self._qlayers

    def _state(self, t_id):
        """ONE pass over the cached layer list per call: (fingerprint of everything that changes which kernels a forward
        launches - per-layer quant state, weight / activation bit widths, smooth-quant switch -, the smooth-quant
        time-range of the forward, whether some layer keeps host-visible running state).  The attributes are plain
        Python fields that scripts also set directly (quant_txt2img.py:297-300), so they are read, not tracked."""
        from .qdiff.models.quant_layer import find_interval
        fp, rng, running = [], None, False
        for m in self._layers():
            sq = bool(getattr(m, "smooth_quant", False))
            fp.append((m.weight_quant, m.act_quant, m.weight_quantizer.n_bits, m.act_quantizer.n_bits, sq))
            if sq and rng is None and hasattr(m, "timerange"):
                # from ``timestep_id`` when the call passes one (QuantModel.forward), else from the state the script set
                # on the layers (set_timestep_id_for_quantlayer)
                rng = find_interval(m.timerange, int(t_id)) if t_id is not None else int(m._range_and_alpha()[0])
            if getattr(m, "smooth_quant_running_stat", False) and "momentum" in str(getattr(m, "channel_wise_scale_type", "")):
                # a RUNNING smooth-quant statistic at inference (the released t2i W4A8 plan leaves it on for
                # blocks.27.mlp.fc2, quant_txt2img.py:297-300) updates host-visible state in every forward: not capturable
                running = True
        return hash(tuple(fp)), rng or 0, running

    def __call__(self, x, t, y, **kwargs):
        from .qdiff.models.quant_layer import PACK_EPOCH
        if not x.is_cuda:
            return self.fn(x, t, y, **kwargs)
        fingerprint, rng, running = self._state(kwargs.get("timestep_id"))
        if running:
            return self.fn(x, t, y, **kwargs)
        if self._epoch != PACK_EPOCH[0]:
            self.graphs.clear()                          # captured graphs reference re-packed weight buffers
            self._epoch = PACK_EPOCH[0]
        kw = {k: v for k, v in kwargs.items() if k != "timestep_id"}
        key = (tuple(x.shape), str(x.dtype), tuple(t.shape), str(t.dtype), tuple(y.shape), str(y.dtype), _ident(kw),
               rng, fingerprint)
        g = self.graphs.get(key)
        if g is None:
            if len(self.graphs) >= self.max_graphs:
                self.graphs.clear()
            g = self.graphs[key] = ForwardGraph(self.fn, x, t, y, kwargs)
            if self._epoch != PACK_EPOCH[0]:             # the first pass packed weights: the capture came after it
                self._epoch = PACK_EPOCH[0]
        return g.run(x, t, y).clone()


class _CounterStepGraph:
    """A fused sampling loop as ONE captured step: {forward(x_model, t, ...), the solver's fused step(step=counter),
    ops.dpmpp_advance} recorded once as a linear chain and replayed for every timestep.  What changes from step to step
    lives in device memory: the latent ``x``, its duplicated copy ``xm`` in the model's dtype, the model-input time ``t``,
    and a counter ``step`` that selects the row of the coefficient table ``rows`` uploaded before the loop.  A subclass
    supplies ``_forward()`` and ``_step(eps)`` (with the buffers of its own, allocated before this constructor runs) and
    its ``run``.  A forward that moves host-visible state (a running smooth-quant statistic) cannot be captured and is
    refused."""

    def __init__(self, fn, kwargs, x, rows, t_first: float, model_dtype, warmup: int, copies: int = 2, first=None):
        """``copies``: how many times ``xm`` and ``t`` hold the n samples (2: one duplicated-batch forward; 1: forwards of
        n samples).  ``first``: a call made once, and waited for, before the warm-up passes (_capture)."""
        from ._lib import VQError
        if GraphedModel(fn)._state(kwargs.get("timestep_id"))[2]:
            raise VQError("%s: a layer keeps a running smooth-quant statistic; its forward is not capturable"
                          % type(self).__name__)
        n = x.shape[0]
        dev = x.device
        self.steps, self.t_first, self.copies = rows.shape[0], float(t_first), copies
        self.rows = rows.to(dev)
        self.x = x.float().contiguous().clone()
        self.xm = torch.cat([self.x] * copies).to(model_dtype)
        self.t = torch.full((copies * n,), self.t_first, dtype=torch.float32, device=dev)
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)
        self.graph = self._capture_step(warmup, first)   # (the counter and the time are reset by every loop, not here)

    def _capture_step(self, warmup, first=None):
        """One {forward, step, advance} of the buffers' current state, recorded."""
        from . import ops

        def one():
            self._step(self._forward())
            ops.dpmpp_advance(self.step, self.rows, self.t)

        return _capture(one, warmup + 1, first=first)[0]

    def _refuse_output(self, entry_point):
        from ._lib import VQError
        raise VQError("%s: %s does not take this model output" % (type(self).__name__, entry_point))

    def _reset(self, x):
        """The state a loop starts from: the latent ``x`` [n, ...] in ``x`` and ``xm``, the first time, the counter at 0."""
        n = self.x.shape[0]
        self.x.copy_(x)
        for q in range(self.copies):
            self.xm[q * n:(q + 1) * n].copy_(x)
        self.t.fill_(self.t_first)
        self.step.zero_()

    def _loop(self, x, before=None, after=None):
        """Start from the latent ``x`` [n, ...] and replay every step; ``before(k)`` / ``after(k)`` around replay k."""
        self._reset(x)
        for k in range(self.steps):
            if before is not None:
                before(k)
            self.graph.replay()
            if after is not None:
                after(k)


class DPMStepGraph(_CounterStepGraph):
    """The guided DPM-Solver++ multistep loop of t2i/dpm_solver.py in the counter form: the step is ops.cfg_dpmpp_step,
    whose x0 history is one more device buffer."""

    def __init__(self, fn, text, kwargs, x, rows, t_first: float, model_dtype=torch.float32, warmup: int = 2):
        self.fn, self.text, self.kwargs = fn, text, kwargs
        self.hist = torch.zeros((3, x.numel()), dtype=torch.float32, device=x.device)
        super().__init__(fn, kwargs, x, rows, t_first, model_dtype, warmup)

    def _forward(self):
        return self.fn(self.xm, self.t, self.text, **self.kwargs)

    def _step(self, eps):
        from . import ops
        if not ops.cfg_dpmpp_step_ok(eps, self.x):
            self._refuse_output("vq_cfg_dpmpp_step")
        ops.cfg_dpmpp_step(eps, self.x, self.hist, self.rows, 0, step=self.step, x_out=self.x, x_model=self.xm)

    @torch.no_grad()
    def run(self, x, step_callback=None):
        self._loop(x, after=None if step_callback is None else lambda k: step_callback(k + 1, self.x.clone()))
        return self.x.clone()


class DDPMStepGraph(_CounterStepGraph):
    """The fused IDDPM loop of t2i/iddpm.py in the counter form: the step is ops.cfg_ddpm_step.  Its noise lives in a
    static buffer of the duplicated shape, which ``run`` refills eagerly before each replay - from ``noise_steps`` or with
    the draw the eager-launched loop makes - so a replay is bit-identical to that loop."""

    def __init__(self, fn, y, mask, kwargs, x, rows, t_first: float, model_dtype=torch.float32, guided: int = 3,
                 warmup: int = 2):
        self.fn, self.y, self.mask, self.kwargs, self.guided = fn, y, mask, kwargs, guided
        self.x0 = torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device)
        self.noise = torch.zeros((2 * x.shape[0],) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
        super().__init__(fn, kwargs, x, rows, t_first, model_dtype, warmup)

    def _forward(self):
        return self.fn(self.xm, self.t, self.y, self.mask, **self.kwargs)

    def _step(self, eps):
        from . import ops
        if not ops.cfg_ddpm_step_ok(eps, self.x):
            self._refuse_output("vq_cfg_ddpm_step")
        ops.cfg_ddpm_step(eps, self.x, self.noise[:self.x.shape[0]], self.rows, 0, step=self.step, x_out=self.x,
                          x0_out=self.x0, x_model=self.xm, guided=self.guided)

    @torch.no_grad()
    def run(self, x, noise_steps=None, generator=None, step_callback=None):
        """``x``: the duplicated start latent [2n, ...] (its first half is read) -> ``cat([x, x])`` of the sample."""
        def refill(k):
            if noise_steps is not None:
                self.noise.copy_(noise_steps[k])
            else:
                self.noise.normal_(generator=generator)

        self._loop(x[:self.x.shape[0]], before=refill, after=None if step_callback is None else
                   lambda k: step_callback(self.steps - 1 - k, self.x.clone(), self.x0.clone()))
        return torch.cat([self.x, self.x])



class SAStepGraph(_CounterStepGraph):
    """The fused SA-Solver PEC loop of t2i/sa_solver.py in the counter form: the step is ops.cfg_sa_step.  Beside the
    corrected latent ``x`` it keeps the predicted one ``xp`` (what the model saw; the result after the last replay), the
    two-slot x0 history and the two-slot noise ring, of which ``run`` refills slot (k + 1) % 2 eagerly before replay k -
    from ``noise_steps`` or with the draw the eager-launched loop makes - so a replay is bit-identical to that loop."""

    def __init__(self, fn, text, kwargs, x, rows, t_first: float, model_dtype=torch.float32, warmup: int = 2):
        self.fn, self.text, self.kwargs = fn, text, kwargs
        self.hist = torch.zeros((2, x.numel()), dtype=torch.float32, device=x.device)
        self.noise = torch.zeros((2,) + tuple(x.shape), dtype=torch.float32, device=x.device)
        self.xp = x.float().contiguous().clone()
        super().__init__(fn, kwargs, x, rows, t_first, model_dtype, warmup)

    def _forward(self):
        return self.fn(self.xm, self.t, self.text, **self.kwargs)

    def _step(self, eps):
        from . import ops
        if not ops.cfg_sa_step_ok(eps, self.x):
            self._refuse_output("vq_cfg_sa_step")
        ops.cfg_sa_step(eps, self.x, self.xp, self.hist, self.noise, self.rows, 0, step=self.step, x_out=self.x,
                        xp_out=self.xp, x_model=self.xm)

    @torch.no_grad()
    def run(self, x, noise_steps=None, generator=None):
        """``noise_steps``: [1 + steps, ...], entry 0 unused (the draw the loop makes before its first model call), or the
        1 + steps draws are made here, from ``generator`` when given."""
        def draw(i, out=None):
            if noise_steps is not None:
                return None if out is None else out.copy_(noise_steps[i])
            return (torch.empty_like(self.x) if out is None else out).normal_(generator=generator)

        draw(0)
        self.xp.copy_(x)
        self._loop(x, before=lambda k: draw(k + 1, self.noise[(k + 1) % 2]))
        return self.xp.clone()


class _RangedStepGraph(_CounterStepGraph):
    """What the STDiT one-graph loops share.  The smooth-quant time range of a forward is host state that a capture bakes
    in, so there is one capture per range the schedule visits (GraphedSampler._range_of), ALL taken in the constructor,
    before the first replay; the warm-up passes move x, xm, t, the counter and whatever else the step keeps, which are
    reset afterwards (``_clear`` for the subclass's own buffers).  ``t_vals``: the model-input time of every call, which a
    QuantModel also receives as ``timestep_id``; ``_forward(serial)`` reads the one being captured from ``self.t_id``.
    ``split``: two forwards of n samples (the second chain forked onto ``self.side``) instead of one joint forward."""

    def __init__(self, net, kwargs, x, rows, t_vals, model_dtype, warmup, split):
        from .qdiff.models.quant_model import QuantModel
        self.side = torch.cuda.Stream() if split else None
        ranged = GraphedSampler(net, None, None, None) if isinstance(net, QuantModel) else None
        self.range_of = [0 if ranged is None else ranged._range_of(t) for t in t_vals]
        self.t_id = t_vals[0]
        # the first pass on ONE stream: it packs weights and fills the module-level caches (StepGraph)
        super().__init__(net.forward, dict(kwargs, timestep_id=t_vals[0]), x, rows, t_vals[0], model_dtype, warmup,
                         copies=1 if split else 2, first=lambda: self._forward(serial=True))
        self.graphs = {self.range_of[0]: self.graph}
        for k, r in enumerate(self.range_of):
            if r not in self.graphs:
                self.t_id = t_vals[k]
                self.graphs[r] = self._capture_step(warmup, first=lambda: self._forward(serial=True))
        self._clear()
        self._reset(x)

    def _clear(self):
        pass

    def _select(self, k):
        self.graph = self.graphs[self.range_of[k]]


class VideoDPMStepGraph(_RangedStepGraph):
    """The fused DPM-Solver++ loop of t2v/dpm_solver.py in the counter form: {forward(patch_major=True) - once for the
    joint route, twice for cfg_split, the two chains forked onto a side stream as StepGraph._forward does -,
    ops.cfg_dpmpp_step_patch(step=counter), ops.dpmpp_advance}, one capture per smooth-quant time range
    (_RangedStepGraph).  ``solver``: a t2v.dpm_solver.VideoDPMSolverPP; ``t_vals``: the model-input time of every call."""

    def __init__(self, solver, x, rows, t_vals, warmup: int = 2):
        self.solver, self.patch = solver, tuple(solver.net.patch_size)
        self.hist = torch.zeros((3, x.numel()), dtype=torch.float32, device=x.device)
        super().__init__(solver.net, solver.model_kwargs, x, rows, t_vals, solver.model_input_dtype, warmup,
                         solver.cfg_split)

    def _clear(self):
        self.hist.zero_()

    def _forward(self, serial=False):
        return self.solver._forward_patch(self.xm, self.t, self.t_id, side=None if serial else self.side)

    def _step(self, eps):
        from . import ops
        if not ops.cfg_dpmpp_step_patch_ok(eps[0], eps[1], self.x, self.patch):
            self._refuse_output("vq_cfg_dpmpp_step_patch")
        ops.cfg_dpmpp_step_patch(eps[0], eps[1], self.x, self.hist, self.rows, 0, self.patch, step=self.step, x_out=self.x,
                                 x_model=self.xm)

    @torch.no_grad()
    def run(self, x, step_callback=None):
        self._loop(x, before=self._select,
                   after=None if step_callback is None else lambda k: step_callback(k + 1, self.x.clone()))
        return self.x.clone()


class VideoDDIMStepGraph(_RangedStepGraph):
    """The fused DDIM loop of t2v/iddpm.py in the counter form: {forward(patch_major=True) - once for the joint route,
    twice for cfg_split -, ops.cfg_ddim_step_patch(step=counter), ops.dpmpp_advance}, one capture per smooth-quant time
    range (_RangedStepGraph).  PTQD's ``ks`` rides in the table.  ``sampler``: a t2v.iddpm.IDDPM; ``model_args``: what
    ddim_sample_loop takes.  A model with ``timestep_wise_mp`` is refused: the host switches it between steps."""

    def __init__(self, sampler, model, x, model_args, ks=None, warmup: int = 2):
        from ._lib import VQError
        from .t2v.iddpm import _accepts_timestep_id
        if getattr(model, "timestep_wise_mp", False):
            raise VQError("VideoDDIMStepGraph: timestep_wise_mp switches the model on the host between steps; "
                          "use ddim_sample_loop(fused=True)")
        n = x.shape[0]
        y = model_args["y"]
        self.model, self.patch = model, tuple(model.patch_size)
        self.split = bool(getattr(model, "cfg_split", False))
        self.texts = (y[:n], y[n:]) if self.split else torch.cat([y[:n], y[n:]], 0)
        self.kw = {k: v for k, v in model_args.items() if k != "y"}
        self.takes_id = _accepts_timestep_id(model)
        self.indices = list(range(sampler.num_timesteps))[::-1]
        t_vals = [sampler.timestep_map[i] for i in self.indices]
        super().__init__(model, self.kw, x, sampler.ddim_rows(sampler.cfg_scale, ks), t_vals,
                         getattr(model, "dtype", torch.float32), warmup, self.split)

    def _forward(self, serial=False):
        from .t2v.iddpm import patch_forward_pair
        kw = dict(self.kw, timestep_id=self.t_id) if self.takes_id else self.kw
        return patch_forward_pair(self.model, self.xm, self.t, self.texts, self.split, kw,
                                  side=None if serial else self.side)

    def _step(self, eps):
        from . import ops
        if not ops.cfg_ddim_step_patch_ok(eps[0], eps[1], self.x, self.patch):
            self._refuse_output("vq_cfg_ddim_step_patch")
        ops.cfg_ddim_step_patch(eps[0], eps[1], self.x, self.rows, 0, self.patch, step=self.step, x_out=self.x,
                                x_model=self.xm)

    @torch.no_grad()
    def run(self, x, step_callback=None):
        """``step_callback(i, x)`` with the loop index of ddim_sample_loop (num_timesteps - 1 down to 0)."""
        self._loop(x, before=self._select,
                   after=None if step_callback is None else lambda k: step_callback(self.indices[k], self.x.clone()))
        return self.x.clone()
