"""The cases of test_block_trace_gpu.py: tiny models (hidden 64, 4 heads, 2 blocks; the builders of the existing GPU tests),
one or two forwards each, behind the route switches of viditq_amd.t2v.stdit.  tests/golden/make_block_traces.py runs them
on the commit whose launches are to be kept and writes tests/golden/fused_block_traces.json; the test replays them.

A case is ``(name, builder, switches)``: ``builder(dev)`` returns a function that runs the traced forwards and returns
their outputs; ``switches`` are module globals of stdit set for the whole case (everything else stays at its default, so
the cases mean the same whatever VQ_* variables the environment holds)."""
import hashlib
import json
import os

import torch

from helpers import FP_LAYERS, GOLD, load_npz, quant_params_of, trace_ops

FIXTURE = os.path.join(GOLD, "fused_block_traces.json")

# every route switch, at the value the cases start from (the defaults of t2v/stdit.py)
DEFAULTS = dict(_ATTN_QUANT=True, _GELU_QUANT=True, _STATIC_FUSED=True, _ATTN_QUANT_JOINT=False, _SMOOTH_JOINT=False,
                _STATIC_ATTN_QUANT=False, _STATIC_FWD_ATTN_QUANT=False, _STATIC_GEMM_QUANT=False,
                _RUNNING_SMOOTH_DEVICE=False, EXACT_KV_EPS_FILL=True)

W4A8_SMOOTH = dict(alpha=[0.11, 0.11], timerange=[[0, 500], [501, 1000]])


def _io(g, dev):
    return g["x"].to(dev), g["y"].half().to(dev), g["mask"].to(dev)


# ---------------------------------------------------------------------------------------------------- STDiT
def _stdit_forward(qnn, x, y, mask, tvs, joint):
    def run():
        outs = []
        for tv in tvs:
            t = tv.to(x.device) if torch.is_tensor(tv) else torch.tensor([tv], device=x.device)
            t = torch.cat([t, t]) if joint else t
            outs.append(qnn(torch.cat([x, x]), t, y, mask=mask) if joint else qnn(x, t, y[:1], mask=mask))
        return outs
    return run


def stdit_w8a8(joint=False, cache_prompt=False, n=1):
    def build(dev):
        from test_model_gpu import _build
        g = load_npz("tiny_stdit_w8a8.npz")
        qnn = _build(g, dev, 8)
        if cache_prompt:
            qnn.model.set_prompt_cache(True)          # the second forward reuses every block's prompt K / V
        return _stdit_forward(qnn, *_io(g, dev), [g["t"]] * n, joint)
    return build


def stdit_w4a8(joint=False, tvs=(721,), running=False):
    def build(dev):
        from test_model_gpu import _build
        g = load_npz("tiny_stdit_w4a8.npz")
        qnn = _build(g, dev, 4, smooth=W4A8_SMOOTH, mixed_precision=[4, 6, 8])
        qnn.set_layer_smooth_quant(model=qnn, module_name_list=FP_LAYERS, smooth_quant=False, smooth_quant_running_stat=False)
        if running:
            qnn.set_layer_smooth_quant(model=qnn, module_name_list=["blocks.1.mlp.fc2"], smooth_quant=True,
                                       smooth_quant_running_stat=True)
        return _stdit_forward(qnn, *_io(g, dev), list(tvs), joint)
    return build


def stdit_w6a6_joint(dev):
    from test_temporal_shared_quant_gpu import _tiny_w6a6_joint
    _, qnn, args, kw = _tiny_w6a6_joint(dev)
    return lambda: [qnn(*args, **kw)]


def stdit_static(joint=True):
    def build(dev):
        from test_static_quant_gpu import _tiny_static_stdit
        qnn, (x2, t2, y), kw = _tiny_static_stdit(dev)
        if joint:
            return lambda: [qnn(x2, t2, y, **kw)]
        return lambda: [qnn(x2[:1], t2[:1], y[:1], **kw)]
    return build


def stdit_frames(T, bits):
    def build(dev):
        from test_long_video_gpu import _inputs, _tiny
        _, qnn = _tiny(dev, bits, T=T)
        x, y, mask = _inputs(dev, T)
        return lambda: [qnn(x, torch.tensor([500], device=dev), y[:1], mask=mask)]
    return build


# ---------------------------------------------------------------------------------------------------- PixArt
def pixart_alpha(plan, b1=False):
    def build(dev):
        from test_parity_gpu import _cfgs, _load_qp, _pixart
        g = load_npz("tiny_pixart_alpha.npz")
        wq, aq = _cfgs(8, T=1, S=64) if plan == "w8a8" else _cfgs(8, dynamic=False, per_group=False, T=1, S=64)
        qnn = _pixart("PixArt", g, dev, wq, aq)
        _load_qp(qnn, quant_params_of(g, "qp" if plan == "w8a8" else "qp_naive"))
        assert all(b.fused_ok() for b in qnn.model.blocks)
        (x, y, mask), t = _io(g, dev), g["t"].to(dev)
        if b1:
            return lambda: [qnn(x[:1], t[:1], y[:1], mask=mask[:1])]
        return lambda: [qnn(x, t, y, mask=mask)]
    return build


def pixart_w4a8(running, tvs):
    """PixArt-MS, 4-bit weights, a smoothing vector on blocks.1.mlp.fc2 - from a fixed statistic, or from one that keeps
    running (test_running_smooth_gpu._tiny_pixart)."""
    def build(dev):
        from test_parity_gpu import _cfgs, _load_qp, _pixart
        g = load_npz("tiny_pixart_w4a8.npz")
        wq, aq = _cfgs(4, T=1, S=64, smooth=dict(alpha=0.3), mixed_precision=[4, 6, 8])
        qnn = _pixart("PixArtMS", g, dev, wq, aq)
        qnn.set_smooth_quant(smooth_quant=False, smooth_quant_running_stat=False)
        qnn.set_layer_smooth_quant(model=qnn, module_name_list=["blocks.1.mlp.fc2"], smooth_quant=True,
                                   smooth_quant_running_stat=running)
        _load_qp(qnn, quant_params_of(g, "qp_after_ptq"))
        x, y, mask = _io(g, dev)
        return lambda: [qnn(x, torch.tensor([tv, tv], device=dev), y, mask=mask) for tv in tvs]
    return build


def _on(*names):
    return {n: True for n in names}


CASES = [
    # STDiT, B = 1 (block 0 takes the temporal position embedding in every STDiT case)
    ("stdit/w8a8/b1", stdit_w8a8(), {}),
    ("stdit/w4a8_smooth/b1_t721_t300", stdit_w4a8(tvs=(721, 300)), {}),
    ("stdit/static_tw/b1", stdit_static(joint=False), {}),
    ("stdit/w8a8_T16/b1", stdit_frames(16, 8), {}),
    ("stdit/w8a8_T33/b1", stdit_frames(33, 8), {}),
    ("stdit/w6a6_T33/b1", stdit_frames(33, 6), {}),
    ("stdit/w8a8/b1/attn_quant_off", stdit_w8a8(), dict(_ATTN_QUANT=False)),
    ("stdit/w8a8/b1/gelu_quant_off", stdit_w8a8(), dict(_GELU_QUANT=False)),
    ("stdit/w8a8/b1/exact_kv_eps_fill_off", stdit_w8a8(), dict(EXACT_KV_EPS_FILL=False)),
    ("stdit/w4a8_smooth/b1/exact_kv_eps_fill_off", stdit_w4a8(), dict(EXACT_KV_EPS_FILL=False)),
    ("stdit/w8a8/b1/prompt_cache_two_forwards", stdit_w8a8(cache_prompt=True, n=2), {}),
    # STDiT, joint (B = 2)
    ("stdit/w8a8/joint", stdit_w8a8(joint=True), {}),
    ("stdit/w8a8/joint/attn_quant_joint", stdit_w8a8(joint=True), _on("_ATTN_QUANT_JOINT")),
    ("stdit/w6a6/joint", stdit_w6a6_joint, {}),
    ("stdit/w6a6/joint/attn_quant_joint", stdit_w6a6_joint, _on("_ATTN_QUANT_JOINT")),
    ("stdit/w4a8_smooth/joint", stdit_w4a8(joint=True), {}),
    ("stdit/w4a8_smooth/joint/attn_quant_joint", stdit_w4a8(joint=True), _on("_ATTN_QUANT_JOINT")),
    ("stdit/w4a8_smooth/joint/smooth_joint", stdit_w4a8(joint=True), _on("_SMOOTH_JOINT")),
    ("stdit/w4a8_smooth/joint/attn_quant_joint+smooth_joint", stdit_w4a8(joint=True), _on("_ATTN_QUANT_JOINT", "_SMOOTH_JOINT")),
    # STDiT, the static tensor-wise plan
    ("stdit/static_tw/joint", stdit_static(), {}),
    ("stdit/static_tw/joint/static_attn_quant", stdit_static(), _on("_STATIC_ATTN_QUANT")),
    ("stdit/static_tw/joint/static_fwd_attn_quant", stdit_static(), _on("_STATIC_FWD_ATTN_QUANT")),
    ("stdit/static_tw/joint/static_gemm_quant", stdit_static(), _on("_STATIC_GEMM_QUANT")),
    ("stdit/static_tw/joint/all_three", stdit_static(), _on("_STATIC_ATTN_QUANT", "_STATIC_FWD_ATTN_QUANT", "_STATIC_GEMM_QUANT")),
    ("stdit/static_tw/b1/all_three", stdit_static(joint=False), _on("_STATIC_ATTN_QUANT", "_STATIC_FWD_ATTN_QUANT", "_STATIC_GEMM_QUANT")),
    ("stdit/static_tw/joint/static_fused_off", stdit_static(), dict(_STATIC_FUSED=False)),
    ("stdit/static_tw/joint/static_fused_off+all_three", stdit_static(),
     dict(_on("_STATIC_ATTN_QUANT", "_STATIC_FWD_ATTN_QUANT", "_STATIC_GEMM_QUANT"), _STATIC_FUSED=False)),
    # STDiT, a running statistic on blocks.1.mlp.fc2 (two forwards: the second finds the buffers of the first)
    ("stdit/w4a8_running_fc2/b1", stdit_w4a8(tvs=(721, 300), running=True), {}),
    ("stdit/w4a8_running_fc2/b1/running_smooth_device", stdit_w4a8(tvs=(721, 300), running=True), _on("_RUNNING_SMOOTH_DEVICE")),
    # PixArt
    ("pixart/alpha_w8a8/b2", pixart_alpha("w8a8"), {}),
    ("pixart/alpha_w8a8/b1", pixart_alpha("w8a8", b1=True), {}),
    ("pixart/alpha_w8a8/b2/gelu_quant_off", pixart_alpha("w8a8"), dict(_GELU_QUANT=False)),
    ("pixart/ms_w4a8_smooth_fc2/b2", pixart_w4a8(False, (820, 400)), {}),
    ("pixart/alpha_naive/b2", pixart_alpha("naive"), {}),
    ("pixart/alpha_naive/b2/static_fwd_attn_quant", pixart_alpha("naive"), _on("_STATIC_FWD_ATTN_QUANT")),
    ("pixart/alpha_naive/b2/static_gemm_quant", pixart_alpha("naive"), _on("_STATIC_GEMM_QUANT")),
    ("pixart/alpha_naive/b2/both", pixart_alpha("naive"), _on("_STATIC_FWD_ATTN_QUANT", "_STATIC_GEMM_QUANT")),
    ("pixart/alpha_naive/b2/static_fused_off", pixart_alpha("naive"), dict(_STATIC_FUSED=False)),
    ("pixart/ms_w4a8_running_fc2/b2", pixart_w4a8(True, (820, 400)), {}),
    ("pixart/ms_w4a8_running_fc2/b2/running_smooth_device", pixart_w4a8(True, (820, 400)), _on("_RUNNING_SMOOTH_DEVICE")),
]
NAMES = [c[0] for c in CASES]


def run_case(name, dev):
    """Builds the case's model, sets its switches, runs its forwards under the tracer: (calls as JSON strings, SHA-256 of
    the outputs' bytes)."""
    from viditq_amd.t2v import stdit
    _, build, switches = CASES[NAMES.index(name)]
    saved = {k: getattr(stdit, k) for k in DEFAULTS}
    try:
        for k, v in dict(DEFAULTS, **switches).items():
            setattr(stdit, k, v)
        with torch.no_grad():
            run = build(dev)
            with trace_ops() as calls:
                outs = run()
            torch.cuda.synchronize()
    finally:
        for k, v in saved.items():
            setattr(stdit, k, v)
    h = hashlib.sha256()
    for o in outs:
        h.update(o.detach().cpu().contiguous().numpy().tobytes())
    return [json.dumps(c, sort_keys=True) for c in calls], h.hexdigest()
