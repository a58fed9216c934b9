"""The running smooth-quant statistic on the device (VQ_RUNNING_SMOOTH_DEVICE): kernel, layer step, graph capture, models.

Kernel: vq_act_scale_momentum against the CPU expectations of running_stat_cases.py (which test_running_smooth_cpu.py
proves equal to the reference's statistic), bit for bit.  Layer: QuantLayer.running_stat_step against QuantLayer.forward on
a copy of the layer, bit for bit - statistic, smoothing vector, packed codes, GEMM output - with the packed buffers staying
where they are.  Graph: the step is capturable (no host read) and replays to the eager result.  Model: the released t2i
arrangement (mlp.fc2 of the last block keeps its statistic running) with every block on the fused route, inside the bounds
the layer-by-layer route of the same configuration is held to.
"""
import copy

import pytest
import torch

import running_stat_cases as rc
from helpers import FP_LAYERS, load_npz, quant_params_of, rel_l2, spy_fused

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ 1. kernel
def _run_case(ops, dev, name, check_reference=False):
    xs, init = rc.inputs(name)
    exp = rc.expected(name, xs, init)
    B, n, C = xs[0].shape
    stat = torch.full((2, 1, C), 7.25, device=dev)                     # range 0 is a bystander, range 1 the state
    stat[1, 0] = init.to(dev)
    scratch = torch.full((B * C,), -1, dtype=torch.int32, device=dev)  # 0xFFFFFFFF: the call zeroes it itself
    cur = torch.full((C,), -3.0, device=dev)
    ref = None
    if check_reference:
        from test_running_smooth_cpu import _reference_layer, reference_step
        QL, stub = _reference_layer(C)
        stub._master_weight = lambda: torch.ones(1, C, device=dev)
        if (init != 0).any():
            stub.act_quantizer.act_scale = init.clone().reshape(1, 1, C).to(dev)
    for j, x in enumerate(xs):
        xd = x.to(dev)
        keep = xd.clone()
        if j == 1:
            scratch.fill_(-1)
        ops.act_scale_momentum(xd, stat[1].view(-1), rc.MOMENTUM, scratch=scratch, cur_out=cur)
        got, got_cur = stat[1, 0].cpu(), cur.cpu()
        assert torch.equal(got_cur, exp[j][1]), (name, j, "cur", float((got_cur - exp[j][1]).abs().max()))
        assert torch.equal(got, exp[j][0]), (name, j, "state", float((got - exp[j][0]).abs().max()))
        assert torch.equal(xd.view(torch.int16), keep.view(torch.int16)), "x was written"
        assert bool((stat[0] == 7.25).all()), "the other time range's slice moved"
        if check_reference:
            ref = reference_step(QL, stub, xd)
            assert torch.equal(ref.cpu(), got), (name, j, "torch on the device")
    ops.act_scale_momentum(xs[0].to(dev), stat[1].view(-1), rc.MOMENTUM)          # scratch / cur_out are optional
    assert torch.isfinite(stat).all()


@pytest.mark.parametrize("name", rc.NAMES)
def test_kernel_matches_the_cpu_expectation_bit_for_bit(ops, dev, name):
    _run_case(ops, dev, name)


@pytest.mark.parametrize("name", [n for n in rc.NAMES if "/B1_" in n or "/B2_" in n])
def test_kernel_matches_the_reference_lines_run_on_the_device(ops, dev, name):
    """B in {1, 2}: torch's device mean multiplies by 1 / B, which is the division only where 1 / B is exact."""
    _run_case(ops, dev, name, check_reference=True)


def test_wrapper_refuses_what_the_entry_point_would_misread(ops, dev):
    x = torch.zeros(2, 4, 16, dtype=torch.float16, device=dev)
    with pytest.raises(ops.VQError):
        ops.act_scale_momentum(x, torch.zeros(8, device=dev), 0.95)                       # one entry per channel
    with pytest.raises(ops.VQError):
        ops.act_scale_momentum(x, torch.zeros(16, device=dev), 0.95, scratch=torch.zeros(16, dtype=torch.int32, device=dev))
    with pytest.raises(ops.VQError):
        ops.act_scale_momentum(x, torch.zeros(16, device=dev), 1.5)                       # VQ_EINVAL from the library
    with pytest.raises(ops.VQError):
        ops.act_scale_momentum(x.float(), torch.zeros(16, device=dev), 0.95)


# ------------------------------------------------------------------------------------------------ 2. layer
def _tiny_pixart(dev):
    """test_pixart_w4a8_running_smooth_quant_statistic's set-up: PixArt-MS in miniature, 4-bit weights with grids for
    [4, 6, 8], alpha 0.3, the statistic of blocks.1.mlp.fc2 (K = 256, N = 64) running."""
    from test_parity_gpu import _cfgs, _load_qp, _pixart
    g = load_npz("tiny_pixart_w4a8.npz")
    wq, aq = _cfgs(4, T=1, S=64, smooth=dict(alpha=0.3), mixed_precision=[4, 6, 8])
    qnn = _pixart("PixArtMS", g, dev, wq, aq)
    qnn.set_smooth_quant(smooth_quant=False, smooth_quant_running_stat=False)
    qnn.set_layer_smooth_quant(model=qnn, module_name_list=["blocks.1.mlp.fc2"], smooth_quant=True,
                               smooth_quant_running_stat=True)
    _load_qp(qnn, quant_params_of(g, "qp_after_ptq"))
    return g, qnn


def _layer_inputs(dev, n=3, B=2, tok=64, K=256):
    g = torch.Generator().manual_seed(2718)
    xs = []
    for j in range(n):
        x = torch.nn.functional.gelu(torch.randn(B, tok, K, generator=g) * (1.5 + j), approximate="tanh")
        x[:, :, 7] = 0                                                 # a dead channel: the 1e-5 patch inside the layer
        x[:, :, 100] *= 9.0                                            # an outlier channel: what smooth quant is for
        xs.append(x.half().to(dev))
    return xs


@pytest.fixture(scope="module")
def fc2_layer(dev, ops):
    _, qnn = _tiny_pixart(dev)
    fc2 = qnn.model.blocks[1].mlp.fc2
    assert type(fc2).__name__ == "QuantLayer" and tuple(fc2.weight.shape) == (64, 256)
    assert fc2.weight_quantizer.n_bits == 4 and fc2.smooth_quant and fc2.smooth_quant_running_stat
    assert fc2.running_stat_device_ok()
    fc2.act_quantizer.act_scale = None                                 # from the first-call branch on
    return fc2


def test_layer_step_equals_quantlayer_forward_bit_for_bit(ops, dev, fc2_layer):
    from viditq_amd.qdiff.models.quant_layer import PACK_EPOCH
    lay, ref = copy.deepcopy(fc2_layer), copy.deepcopy(fc2_layer)
    r, alpha = lay._range_and_alpha()
    ptrs, epoch = None, None
    for j, x in enumerate(_layer_inputs(dev)):
        e0 = PACK_EPOCH[0]
        qa, pw = lay.running_stat_step(x)
        e1 = PACK_EPOCH[0]
        out = ops.gemm_i8(qa, pw, bias=lay.bias_f32()).reshape(x.shape[0], x.shape[1], -1)
        want = ref(x)                                                  # QuantLayer.forward: host-visible statistic, re-pack
        a, b = lay.act_quantizer.act_scale, ref.act_quantizer.act_scale
        assert a.shape == b.shape == (1, 1, 256) and torch.equal(a, b), (j, float((a - b).abs().max()))
        assert float(a[0, 0, 7]) > 0                                   # the dead channel was patched / decays, never zero
        s_dev = lay._packed[("run", r, 4)]["s"].reshape(-1)
        s_ref = ref.smooth_vector(r, alpha).reshape(-1)
        assert torch.equal(s_dev, s_ref), j
        assert torch.equal(s_dev, ref.channel_wise_scale(r, alpha).reshape(-1)), j     # recomputed from the updated statistic
        assert torch.equal(s_dev, lay.channel_wise_scale(r, alpha).reshape(-1)), j
        pw_ref = ref.packed_weight(r, ref.smooth_vector(r, alpha))
        assert pw.n_bits == pw_ref.n_bits == 4 and pw.wq.dtype == torch.uint8
        for t, u in zip(pw.tensors(), pw_ref.tensors()):
            assert torch.equal(t, u), j
        assert out.dtype == want.dtype == torch.float16 and torch.equal(out, want), (j, rel_l2(out.float(), want.float()))
        now = [t.data_ptr() for t in pw.tensors()] + [s_dev.data_ptr(), lay.act_quantizer.act_scale.data_ptr()]
        if j == 0:
            ptrs = now
        else:
            assert now == ptrs, "a buffer of the device step moved"
            assert e1 == e0, "PACK_EPOCH moved after the first call"
    assert not torch.equal(lay.act_quantizer.act_scale, torch.zeros_like(a))


def test_layer_step_without_smooth_quant_moves_the_statistic_only(ops, dev, fc2_layer):
    """The ``elif`` branch of QuantLayer.forward: smooth_quant off, statistic running - quantizer and packer without s."""
    lay, ref = copy.deepcopy(fc2_layer), copy.deepcopy(fc2_layer)
    lay.smooth_quant = ref.smooth_quant = False
    for j, x in enumerate(_layer_inputs(dev, n=2)):
        x = x.clone()
        x[:, :, 7] = 0.5                                               # (no zero column: the reference patches under smooth_quant only)
        qa, pw = lay.running_stat_step(x)
        out = ops.gemm_i8(qa, pw, bias=lay.bias_f32()).reshape(x.shape[0], x.shape[1], -1)
        want = ref(x)
        assert torch.equal(lay.act_quantizer.act_scale, ref.act_quantizer.act_scale), j
        assert torch.equal(out, want), j
        for t, u in zip(pw.tensors(), ref.packed_weight(0).tensors()):
            assert torch.equal(t, u)


# ------------------------------------------------------------------------------------------------ 3. graph
def test_layer_step_is_capturable_and_replays_to_the_eager_result(ops, dev, fc2_layer):
    lay, eager = copy.deepcopy(fc2_layer), copy.deepcopy(fc2_layer)
    xs = _layer_inputs(dev)
    xbuf = xs[0].clone()

    def step(layer, x):
        qa, pw = layer.running_stat_step(x)
        return ops.gemm_i8(qa, pw, bias=layer.bias_f32())

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(lay, xbuf)                                                # warm-up: allocates the fixed buffers
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                      # a host read of device data would fail the capture
        out = step(lay, xbuf)
    stat = lay.act_quantizer.act_scale
    stat.zero_()                                                       # (in place: the graph holds its address)
    got = []
    for x in xs:
        xbuf.copy_(x)
        graph.replay()
        got.append((out.clone(), stat.clone()))
    eager.act_quantizer.act_scale = None
    for j, x in enumerate(xs):
        want = step(eager, x)
        assert torch.equal(got[j][1], eager.act_quantizer.act_scale), (j, "statistic")
        assert torch.equal(got[j][0], want), (j, "output")
    assert not torch.equal(got[0][0], got[1][0])


# ------------------------------------------------------------------------------------------------ 4. models
@pytest.mark.parametrize("route", ["device", "layerwise"])
def test_pixart_w4a8_running_statistic_on_the_fused_route(ops, dev, parity, monkeypatch, route):
    """BASELINE config 5 in miniature, as test_pixart_w4a8_running_smooth_quant_statistic runs it - with the switch on every
    block takes forward_fused.  Both routes are held to that test's bounds and recorded side by side.
    Achieved figures go to the session's parity record under the keys tiny_pixart_w4a8_running_<route>/call<j>_t<t>."""
    from test_parity_gpu import _rec
    from viditq_amd import t2i
    from viditq_amd.t2v import stdit
    monkeypatch.setattr(stdit, "_RUNNING_SMOOTH_DEVICE", route == "device")
    g, qnn = _tiny_pixart(dev)
    blk = qnn.model.blocks[1]
    assert qnn.model.blocks[0].fused_ok() and not blk.fused_ok()       # fused_ok() itself is what it was
    assert blk.fused_running_ok() and stdit.takes_fused(blk) == (route == "device")
    fc2 = blk.mlp.fc2
    x, y, mask = g["x"].to(dev), g["y"].half().to(dev), g["mask"].to(dev)
    for j, tv in enumerate((820, 400, 90)):
        with spy_fused(t2i.pixart.PixArtMSBlock) as seen:
            out = qnn(x, torch.tensor([tv, tv], device=dev), y, mask=mask).cpu().float()
        assert len(seen) == (2 if route == "device" else 1)
        a, b = fc2.act_quantizer.act_scale.cpu().float(), g["act_scale_after_call%d" % j]
        print("call %d t=%d act_scale max rel dev %.3e" % (j, tv, float(((a.reshape(b.shape) - b).abs() / (b.abs() + 1e-4)).max())))
        e = _rec(parity, "tiny_pixart_w4a8_running_%s/call%d_t%d" % (route, j, tv), out, g["w4a8_call%d_t%d" % (j, tv)])
        print(route, j, tv, e)
        assert torch.allclose(a.reshape(b.shape), b, rtol=2e-2, atol=1e-4)
        assert e["vs_ref_fp32"] < 5.2e-3, e
    assert qnn.check_status() == 0


def test_stdit_block_with_running_fc2_statistic_fused_equals_layerwise(ops, dev, monkeypatch):
    """One tiny STDiT block (W4A8, two time ranges) whose mlp.fc2 keeps its statistic running: the fused route under the switch
    against the layerwise route of a copy, under the tolerance between routes of test_tiny_stdit_layerwise_equals_fused."""
    from test_model_gpu import _build
    from viditq_amd.t2v import stdit
    g = load_npz("tiny_stdit_w4a8.npz")
    qnn = _build(g, dev, 4, smooth=dict(alpha=[0.11, 0.11], timerange=[[0, 500], [501, 1000]]), mixed_precision=[4, 6, 8])
    qnn.set_layer_smooth_quant(model=qnn, module_name_list=FP_LAYERS, smooth_quant=False, smooth_quant_running_stat=False)
    qnn.set_layer_smooth_quant(model=qnn, module_name_list=["blocks.1.mlp.fc2"], smooth_quant=True,
                               smooth_quant_running_stat=True)
    blk = qnn.model.blocks[1]
    assert not blk.fused_ok() and blk.fused_running_ok() and qnn.model.blocks[0].fused_ok()
    lw = copy.deepcopy(blk)
    gen = torch.Generator().manual_seed(99)
    x = torch.randn(1, 64, 64, generator=gen).half().to(dev)
    y = (torch.randn(1, 12, 64, generator=gen) * 0.5).half().to(dev)
    t = (torch.randn(1, 6 * 64, generator=gen) * 0.3).half().to(dev)
    monkeypatch.setattr(stdit, "_RUNNING_SMOOTH_DEVICE", False)
    with spy_fused(stdit.STDiTBlock) as seen:
        want = lw(x, y, t)                                             # flag off: the layerwise route, as before
    assert len(seen) == 0
    monkeypatch.setattr(stdit, "_RUNNING_SMOOTH_DEVICE", True)
    with spy_fused(stdit.STDiTBlock) as seen:
        got = blk(x, y, t)
    assert len(seen) == 1
    a, b = blk.mlp.fc2.act_quantizer.act_scale, lw.mlp.fc2.act_quantizer.act_scale
    err = rel_l2(got.float().cpu(), want.float().cpu())
    print("fused (device statistic) vs layerwise: rel-L2 %.3e, act_scale max abs dev %.3e" % (err, float((a - b).abs().max())))
    assert torch.allclose(a, b, rtol=2e-2, atol=1e-4)
    assert err < 2.5e-3
