"""GELU in front of fc2's quantizer at every call site of rq_gelu_tanh, over every finite fp16 input: one launch of
gelu_cases.rows() per route through ops.gelu_rowquant, held by gelu_cases.check() - the step and zero point of every row
bit for bit (the rows' extremes are pinned inputs), the codes bit for bit on every pinned element and one of two oracle
codes on the unpinned ones (0.3 % of the inputs, fixed on the CPU), R, zero pads, status 0.  test_gelu_cases_cpu.py shows
that a GELU one fp16 ulp off at a single input fails these rows, and that a correct fp32 evaluation cannot.

s is 0.5 in every channel: x / s and x * RN(1 / s) are exact, the row plan carries over with the values doubled (the
per-channel indexing of s is pinned by test_quantizer_edges_gpu.py; here it is the GELU value at each call site).

route (vq_gelu_rowquant_fast / vq_gelu_rowquant_pair_fast's dispatch) -> kernel:
  B = 1, C = 4608                        rowquant_split_kernel<4, true, true>: NF = 4 chunks of 8 and the TAIL8 chunk of 4 per lane
  B = 1, C = 4600 (Kp = 4608)            rowquant_fast_kernel<9, .., GELU>: masked last chunk, pad columns [4600, 4608)
  B = 1, C = 4608, s (>= 64 rows)        rowquant_smooth_lds_kernel<9, GELU>
  B = 1, C = 4608, s, fast_div=False     rowquant_fast_kernel<9, HAS_S, .., GELU>, IEEE division
  B = 1, C = 1152 / 320                  rowquant_fast_kernel<3 / 1, .., GELU>
  B = 1, C = 1152 / 320, s               rowquant_fast_kernel<3 / 1, HAS_S, .., GELU>, reciprocal form
  B = 2, C = 4608                        rowquant_split_kernel<4, true, true, PAIR>
  B = 2, C = 4608, s                     rowquant_smooth_lds_kernel<9, GELU, PAIR>
  B = 2, C = 1152                        rowquant_fast_kernel<3, .., GELU, PAIR>
  B = 2, C = 1152, s                     rowquant_fast_kernel<3, HAS_S, .., GELU, PAIR>
Every route at 8 bits; both un-smoothed B = 1 routes at C = 4608 / 4600 and the un-smoothed PAIR route at C = 1152 at 6 bits
as well (the clamp arm of RQ_BY_WIDTH behind the GELU, a four times coarser grid with its own plan)."""
import functools

import pytest
import torch

import gelu_cases as gc

pytestmark = pytest.mark.gpu

# kernel, B, C, s, fast_div, n_bits
ROUTES = [
    ("split<4,TAIL8>", 1, 4608, None, True, 8), ("split<4,TAIL8>", 1, 4608, None, True, 6),
    ("fast<9> pad columns", 1, 4600, None, True, 8), ("fast<9> pad columns", 1, 4600, None, True, 6),
    ("smooth_lds<9>", 1, 4608, 0.5, True, 8), ("fast<9,HAS_S> IEEE division", 1, 4608, 0.5, False, 8),
    ("fast<3>", 1, 1152, None, True, 8), ("fast<3,HAS_S>", 1, 1152, 0.5, True, 8),
    ("fast<1>", 1, 320, None, True, 8), ("fast<1,HAS_S>", 1, 320, 0.5, True, 8),
    ("split<4,TAIL8,PAIR>", 2, 4608, None, True, 8), ("smooth_lds<9,PAIR>", 2, 4608, 0.5, True, 8),
    ("fast<3,PAIR>", 2, 1152, None, True, 8), ("fast<3,PAIR>", 2, 1152, None, True, 6),
    ("fast<3,HAS_S,PAIR>", 2, 1152, 0.5, True, 8),
]


@functools.lru_cache(maxsize=2)
def _expected(n_bits, B, C, s):
    x = gc.rows(n_bits, B, C)
    return x, gc.expected(x, n_bits, s)


@pytest.mark.parametrize("kernel,B,C,s,fast_div,n_bits", ROUTES,
                         ids=["%s-B%d-C%d-%s-b%d" % (r[0].replace(" ", "_"), r[1], r[2], "s" if r[3] else "plain", r[5]) for r in ROUTES])
def test_gelu_rowquant_exact(ops, dev, kernel, B, C, s, fast_div, n_bits):
    x, exp = _expected(n_bits, B, C, s)
    n_tok = x.shape[1]
    assert n_tok >= 64
    sd = None if s is None else torch.full((C,), s, dtype=torch.float32, device=dev)
    if sd is not None and fast_div:
        assert ops.smooth_rcp(sd) is not None
    st = ops.new_status(dev)
    qa = ops.gelu_rowquant(x.to(dev), n_bits=n_bits, s=sd, status=st, fast_div=fast_div)
    assert qa.xq.shape == (B * n_tok, ops.pad128(C))
    got = {"xq": qa.xq.cpu(), "sx": qa.sx.cpu(), "zx": qa.zx.cpu(), "R": qa.R.cpu(), "status": int(st.item()),
           "zpf": None if qa.zpf is None else qa.zpf.cpu()}
    unp = ~exp["pinned"]
    other = int((unp & (got["xq"][:, :C] != exp["xq"][:, :C])).sum())
    print("%s B%d C%d b%d: %d rows, %d unpinned elements (%.3g), %d of them on their other admissible code"
          % (kernel, B, C, n_bits, B * n_tok, int(unp.sum()), float(unp.double().mean()), other))
    gc.check(exp, got, "%s B%d C%d b%d" % (kernel, B, C, n_bits))
