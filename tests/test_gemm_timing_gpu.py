"""The GEMM_TIMING bracket of ops.gemm_i8 and ops.gemm_i8_rowquant_static (bench.py's live roofline measurement): with a
list in the global each launch appends exactly one (start event, end event, int8 ops, algorithmic bytes); with None
nothing is recorded.  The two byte models differ on purpose and are written out by hand here."""
import pytest
import torch

pytestmark = pytest.mark.gpu

M, N, K = 16, 128, 128


def _operands(ops, dev):
    g = torch.Generator().manual_seed(5)
    xs = torch.randint(-100, 101, (M, K), generator=g, dtype=torch.int8)
    ws = torch.randint(-100, 101, (N, K), generator=g, dtype=torch.int8)
    zx = torch.zeros(M, dtype=torch.int32)
    qa = ops.QAct(xs.to(dev), torch.full((M,), 2.0 ** -10).to(dev), zx.to(dev), xs.int().sum(1).int().to(dev), K, 8)
    pw = ops.PackedWeight(ws.to(dev), torch.full((N,), 2.0 ** -10).to(dev), torch.zeros(N, dtype=torch.int32, device=dev),
                          ws.int().sum(1).int().to(dev), N, K, ops.pad128(K), 8)
    return qa, pw


def test_each_gemm_appends_one_bracket_and_none_records_nothing(ops, dev):
    qa, pw = _operands(ops, dev)
    resid = torch.zeros(M, N, dtype=torch.float16, device=dev)
    delta = torch.tensor([2.0 ** -6], dtype=torch.float32, device=dev)
    zp = torch.tensor([64.0], dtype=torch.float32, device=dev)
    assert ops.gemm_rowquant_static_ok(M, N, K, 8, 8)
    assert ops.GEMM_TIMING is None
    timing = []
    try:
        ops.GEMM_TIMING = timing
        ops.gemm_i8(qa, pw, epilogue=ops.EPI_RESID, resid=resid)
        assert len(timing) == 1
        assert ops.gemm_i8_rowquant_static(qa, pw, None, delta, zp, 8) is not None
        assert len(timing) == 2
        ops.GEMM_TIMING = None
        ops.gemm_i8(qa, pw, epilogue=ops.EPI_RESID, resid=resid)
        ops.gemm_i8_rowquant_static(qa, pw, None, delta, zp, 8)
        assert len(timing) == 2
    finally:
        ops.GEMM_TIMING = None
    torch.cuda.synchronize()
    want_bytes = [M * K + N * K + 2 * M * N * 2,                 # codes, 8-bit weights, the fp16 output and the residual
                  M * K + N * K + M * ops.pad128(N) + 12 * M]    # codes, weights, the output codes and three row terms
    for rec, nbytes in zip(timing, want_bytes):
        assert isinstance(rec, tuple) and len(rec) == 4
        e0, e1, n_ops, got = rec
        assert isinstance(e0, torch.cuda.Event) and isinstance(e1, torch.cuda.Event)
        assert n_ops == 2 * M * N * K
        assert got == nbytes
        assert e0.elapsed_time(e1) >= 0
