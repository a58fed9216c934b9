"""ops.kv_compress (vq_kv_compress, csrc/kv_compress.hip): PixArt-Sigma key / value compression and q / k LayerNorm in one
launch - the kernel against a float64 reference, the entry point's refusals, and the route through the tiny PixArt."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import kv_compress_cases as kc
from helpers import load_npz, quant_params_of, rel_l2, state_dict_of

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("C", [64, 1152])
@pytest.mark.parametrize("shape", kc.SHAPES)
@pytest.mark.parametrize("qk_norm", [False, True])
@pytest.mark.parametrize("sampling", ["conv", "uniform", "ave", "uniform_every"])
def test_kernel_against_float64(dev, ops, sampling, qk_norm, shape, C):
    """Picks without qk_norm are bit-equal; arithmetic arms meet kv_compress_cases.check.  The q columns come back
    bit-identical without qk_norm (they are NaN: the kernel does not read them), the guard row stays NaN."""
    B, H, W, sr = shape
    d = kc.make(B, H, W, sr, C, qk_norm)
    q_ref, k_ref, v_ref, extra = kc.reference(d, B, H, W, sr, C, sampling)
    buf = d["buf"].to(dev)
    g = lambda t: None if t is None else (t[0].to(dev), t[1].to(dev), t[2])
    k2, v2 = ops.kv_compress(buf[:B * H * W], B, H, W, C, sr, sampling, d["sr_w"].to(dev), d["sr_b"].to(dev), g(d["norm"]),
                             g(d["k_norm"]), g(d["q_norm"]))
    torch.cuda.synchronize()
    after = buf.cpu()
    assert k2.shape == v2.shape == k_ref.shape
    kc.check(k2.cpu(), k_ref, extra, sampling == "conv" or qk_norm)
    kc.check(v2.cpu(), v_ref, None, sampling == "conv")
    if qk_norm:
        kc.check(after[:-1, :C], q_ref, None, True)
    else:
        assert torch.equal(after[:, :C].view(torch.int16), d["buf"][:, :C].view(torch.int16))
    assert torch.equal(after[:, C:].view(torch.int16), d["buf"][:, C:].view(torch.int16))     # k, v and the guard row


@pytest.mark.parametrize("name,C,H,W,sr,ld_extra,off,code", [
    ("sr = 3", 64, 6, 6, 3, 0, 0, -4), ("H % sr", 64, 5, 4, 2, 0, 0, -2), ("C % 8", 60, 4, 4, 2, 0, 0, -2),
    ("C > 2048", 2056, 4, 4, 2, 0, 0, -4), ("misaligned", 64, 4, 4, 2, 0, 8, -2), ("ld < 3C", 64, 4, 4, 2, -8, 0, -2)])
def test_refusals_launch_nothing(dev, ops, name, C, H, W, sr, ld_extra, off, code):
    """Every case ops.kv_compress_ok refuses (a pointer's alignment is the entry point's alone) returns the documented code
    and leaves the output canary untouched."""
    from viditq_amd import _lib
    ld = 3 * C + ld_extra
    if not off:
        assert not ops.kv_compress_ok(C, H, W, sr, "conv", ld)
    assert ops.kv_compress_ok(64, 4, 4, 2, "conv", 192)
    buf = torch.zeros(H * W * 3 * C + 64, dtype=torch.float16, device=dev)
    vec = torch.ones(C * 16 + 64, dtype=torch.float32, device=dev)
    out = torch.full((2, H * W * C), 7.0, dtype=torch.float16, device=dev)
    rc = _lib.load().vq_kv_compress(buf.data_ptr() + off, ld, *[vec.data_ptr()] * 4, 1e-5, None, None, 0.0, None, None, 0.0,
                                    out[0].data_ptr(), out[1].data_ptr(), 1, H, W, C, sr, _lib.KVC_CONV,
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == code, name
    assert bool((out == 7.0).all())


def _tiny(dev, samp):
    """tests/test_model_gpu.py::test_tiny_pixart_kv_compression_and_qk_norm's model, quantized W8A8, and its inputs."""
    from test_model_gpu import _cfgs
    from viditq_amd.qdiff.models import QuantModel
    from viditq_amd.qdiff.quantizer import BaseQuantizer
    from viditq_amd.t2i import PixArtMS
    g = load_npz("tiny_pixart_kvcompress.npz")
    m = PixArtMS(input_size=16, depth=2, hidden_size=64, num_heads=4, model_max_length=12, caption_channels=32, qk_norm=True,
                 kv_compress_config={"sampling": samp, "scale_factor": 2, "kv_compress_layer": [0, 1]}, dtype=torch.float16)
    assert not m.load_state_dict(state_dict_of(g), strict=False).missing_keys
    wq, aq = _cfgs(8)
    aq["n_spatial_token"], aq["n_temporal_token"] = 64, 1
    qnn = QuantModel(m.half().to(dev).eval(), wq, aq, model_type="pixart")
    qnn.set_module_name_for_quantizer(qnn.model)
    qnn.fp_layer_list = ["x_embedder", "t_embedder", "t_block", "y_embedder", "csize_embedder", "ar_embedder"] + \
        (["attn.sr"] if samp == "conv" else [])                        # (a quantized `attn.sr` raises, as in the reference)
    qp = quant_params_of(g)
    qnn.set_quant_params_dict({mod.module_name: [qp.get(mod.module_name, {}), {}] for mod in qnn.model.modules()
                               if isinstance(mod, BaseQuantizer)})
    qnn.set_quant_init_done("weight")
    qnn.set_quant_init_done("activation")
    qnn.set_quant_state(True, True)
    return qnn, g, (g["x"].to(dev), g["t"].to(dev), g["y"].half().to(dev), g["mask"].to(dev))


@pytest.mark.parametrize("samp", ["ave", "uniform", "uniform_every", "conv"])
def test_model_route(dev, ops, monkeypatch, samp):
    """Switch on: one ops.kv_compress per compressed block per forward, no conv2d / layer_norm of attend, the bounds
    test_tiny_pixart_kv_compression_and_qk_norm holds the torch route to; switch off: no call.  'uniform' also replays the forward from a graph, bit for bit."""
    from viditq_amd import graph
    from viditq_amd.t2i import pixart
    qnn, g, (x, t, y, mask) = _tiny(dev, samp)
    calls = []
    real = ops.kv_compress
    monkeypatch.setattr(ops, "kv_compress", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    qnn(x, t, y, mask=mask)
    assert not calls                                                   # the default: off
    monkeypatch.setattr(pixart, "_KV_COMPRESS_HIP", True)

    def banned(*a, **k):
        raise AssertionError("a torch op of attend ran on the HIP route")
    attend = pixart.AttentionKVCompress.attend

    def guarded(self, *a, **k):                                        # conv2d / layer_norm are banned inside attend only
        with monkeypatch.context() as mp:
            mp.setattr(F, "conv2d", banned)
            mp.setattr(F, "layer_norm", banned)
            return attend(self, *a, **k)
    monkeypatch.setattr(pixart.AttentionKVCompress, "attend", guarded)
    out = qnn(x, t, y, mask=mask)
    assert len(calls) == 2
    if samp == "conv":                                                 # no quantized golden: W8A8 beside an FP compression
        assert rel_l2(out.cpu().float(), g["fp_conv"]) < 0.08
    else:
        drift = rel_l2(g["w8a8_%s_ref_fp16" % samp], g["w8a8_" + samp])
        e = rel_l2(out.cpu().float(), g["w8a8_" + samp])
        assert e < 1.25 * drift + 1e-4, (e, drift)
    assert qnn.check_status() == 0
    if samp == "uniform":
        gm = graph.GraphedModel(qnn.forward, qnn=qnn)
        for _ in range(3):                                             # capture, then replays
            assert torch.equal(gm(x, t, y, mask=mask, timestep_id=int(g["t"][0])), out)     # (a host int: no sync in capture)
