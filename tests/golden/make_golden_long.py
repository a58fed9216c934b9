"""Generate the 64-frame golden vectors by IMPORTING THE REFERENCE (authoring container only).

Run:  python tests/golden/make_golden_long.py        (needs /root/reference; writes tests/golden/tiny_stdit_t64.npz)

The reference's third OpenSORA configuration (t2v/configs/opensora/inference/64x512x512.py) has 64 frames and
time_scale = 2/3.  Pinned here at tiny width: the reference's own QuantModel(STDiT) at input_size = (64, 8, 8),
time_scale = 2/3, hidden 64, 4 heads, depth 2, 12-token prompts, under
  * W8A8 dynamic (cfg_split: one B = 1 forward per chain; the fused attention + attn_temp.proj quantizer path), and
  * W6A6 dynamic (B = 1; plain attention output + the layer's own quantizer),
each one conditional forward in fp32 and in the reference's own fp16 mode (the file stays under 1 MB), plus the fp32 W8A8 DDIM-2 final latent (the reference's fp16-mode
DDIM loop on CPU half kernels stops in QuantLayer's NaN check at 64 frames, so no fp16-mode trajectory is stored).  The state dict carries the
reference's pos_embed_temporal (the 2/3-scaled sin-cos table).  Only data is written; no reference source text.
"""
from __future__ import annotations

import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from oracle import ref_import  # noqa: E402
from make_golden import _ddim, _half_copy, _qp, h, npz  # noqa: E402

TINY64 = dict(input_size=(64, 8, 8), depth=2, hidden_size=64, num_heads=4, model_max_length=12, caption_channels=32,
              time_scale=2 / 3)
FP_LAYERS = ["x_embedder", "t_block", "t_embedder", "y_embedder", "final_layer"]


def build_tiny64(R, seed):
    torch.manual_seed(seed)
    m = R.STDiT(enable_flashattn=False, **TINY64)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in m.named_parameters():      # re-draw zero-initialised tensors so every branch carries signal
            if p.abs().sum() == 0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
        for p in m.parameters():
            p.copy_(h(p))
        for n, b in m.named_buffers():
            b.copy_(h(b))
    m.eval()
    return m


def quant_model(R, m, bits, x, t, y, mask):
    wq = ref_import.wq_cfg(bits, mixed_precision=[4, 6, 8])
    aq = ref_import.aq_cfg(n_bits=bits, T=64, S=16, n_prompt=12)
    qnn = R.QuantModel(m, wq, aq)
    qnn.set_module_name_for_quantizer(qnn.model)
    qnn.fp_layer_list = list(FP_LAYERS)
    qnn.set_quant_state(True, False)
    qnn(x, t, y, mask=mask)                    # weight min-max init (dynamic activations need no calibration)
    qnn.set_quant_init_done("weight")
    qnn.set_quant_init_done("activation")
    qnn.set_quant_state(True, True)
    qnn.cfg_split = True
    return qnn


def tiny_stdit_t64(R):
    out = {}
    m = build_tiny64(R, seed=64)
    for k, v in m.state_dict().items():
        out["sd/" + k] = v.clone()
    g = torch.Generator().manual_seed(65)
    x = h(torch.randn(1, 4, 64, 8, 8, generator=g))
    y = h(torch.randn(2, 1, 12, 32, generator=g) * 0.5)
    mask = torch.zeros(1, 12, dtype=torch.int64)
    mask[0, :9] = 1
    t = torch.tensor([721])
    out["x"], out["y"], out["mask"], out["t"] = x, y, mask, t
    import copy
    with torch.no_grad():
        for bits in (8, 6):
            qnn = quant_model(R, copy.deepcopy(m), bits, x, t, y[:1], mask)
            tag = "w%da%d" % (bits, bits)
            out[tag + "_cond"] = qnn(x, t, y[:1], mask=mask)
            q16 = _half_copy(qnn)
            out[tag + "_cond_ref_fp16"] = q16(x, t, y[:1].half(), mask=mask).float()
            if bits == 8:
                z = h(torch.randn(1, 4, 64, 8, 8, generator=torch.Generator().manual_seed(66)))
                out["ddim_z"] = z
                out["w8a8_ddim2_final"] = _ddim(qnn, 2, z, y, mask)[0]
            del q16
            qp = {}
            _qp(qp, "qp_" + tag, qnn)         # weight grids only (the activation grids are per-forward, dynamic)
            out.update({k: v for k, v in qp.items() if k.endswith(".weight_quantizer/delta")})
    npz("tiny_stdit_t64.npz", **out)


def main():
    assert ref_import.available(), "needs /root/reference"
    torch.set_grad_enabled(False)
    tiny_stdit_t64(ref_import.load())


if __name__ == "__main__":
    main()
