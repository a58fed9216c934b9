"""The private helpers every launch wrapper of viditq_amd.ops takes its operand checks, allocations and pointer tables from
("No fallback"): their contracts, on CPU tensors - none of them calls the library."""
import pytest
import torch


@pytest.fixture
def ops(monkeypatch):
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib, ops as _ops

    def reached(*a, **k):
        raise AssertionError("a helper called the library")
    monkeypatch.setattr(_lib, "load", reached)
    return _ops


def test_qact_empty_shapes_and_types(ops):
    cpu = torch.device("cpu")
    qa = ops._qact_empty(6, 128, 72, 5, cpu, want_zp=True)
    assert isinstance(qa, ops.QAct)
    assert tuple(qa.xq.shape) == (6, 128) and qa.xq.dtype == torch.int8
    for t, dt in ((qa.sx, torch.float32), (qa.zx, torch.int32), (qa.R, torch.int32), (qa.zpf, torch.float32)):
        assert tuple(t.shape) == (6,) and t.dtype == dt and t.device == cpu
    assert qa.K == 72 and qa.n_bits == 5 and qa.rows == 6 and qa.Kp == 128
    assert ops._qact_empty(6, 128, 72, 5, cpu).zpf is None
    five = [qa.xq, qa.sx, qa.zx, qa.R, qa.zpf]
    assert len({t.data_ptr() for t in five}) == 5                       # five tensors, not views of one


def test_tensorwise_grid_names_its_caller(ops):
    one, two = torch.ones(1), torch.ones(2)
    d, z = ops._tensorwise_grid(one, one, "some_wrapper")
    assert d is one and z is one
    for delta, zp in ((two, one), (one, two)):
        with pytest.raises(ops.VQError, match="some_wrapper: a tensor-wise grid"):
            ops._tensorwise_grid(delta, zp, "some_wrapper")


def test_flat_f32_refuses_cpu_and_other_types(ops):
    with pytest.raises(ops.VQError, match="delta must be a GPU tensor"):
        ops._flat_f32(torch.ones(2, 1), "delta")


def test_ptr_array_pads_with_null(ops):
    a = 1 << 20
    arr = ops._ptr_array([a, None], n=3)
    assert len(arr) == 3 and arr[0] == a and arr[1] is None and arr[2] is None
    assert len(ops._ptr_array([a])) == 3 and list(ops._ptr_array([a, a + 16, a + 32])) == [a, a + 16, a + 32]
    qs = [ops._qact_empty(2, 128, 64, 8, torch.device("cpu")) for _ in range(2)]
    tables = ops._qact_tables(qs)
    assert len(tables) == 4
    for table, f in zip(tables, ("xq", "sx", "zx", "R")):
        assert list(table) == [getattr(qs[0], f).data_ptr(), getattr(qs[1], f).data_ptr(), None]
    assert ops._qact_ptrs(qs[0]) == tuple(getattr(qs[0], f).data_ptr() for f in ("xq", "sx", "zx", "R"))


def test_attn_scale(ops):
    assert ops._attn_scale(64, None) == 0.125
    assert ops._attn_scale(64, 2) == 2.0 and isinstance(ops._attn_scale(64, 2), float)
    assert ops._attn_scale(72, None) == float(72) ** -0.5


def test_check_k_and_gpu_refusals(ops):
    cpu = torch.device("cpu")
    a, b = ops._qact_empty(2, 128, 64, 8, cpu), ops._qact_empty(2, 256, 200, 8, cpu)
    ops._check_k(a, a)
    with pytest.raises(ops.VQError, match="K mismatch: activation 64/128 weight 200/256"):
        ops._check_k(a, b)
    with pytest.raises(ops.VQError, match=r"x must be a GPU tensor \(no CPU fallback in the product path\)"):
        ops._req_gpu(a.xq, "x")
    with pytest.raises(ops.VQError, match="q must be a GPU fp16 tensor"):
        ops._req_f16((torch.zeros(2, dtype=torch.float16), "q"))
    assert ops._req_opt(None, torch.float32, "bias") is None


def test_rcp_gate_without_a_vector(ops):
    assert ops._rcp_or_none(None) is None
    assert ops._NO_RCP is not None


def test_check_o_keeps_each_wrappers_rule(ops):
    """On the CPU only the refusal common to all forms is reachable: a CPU output is refused by the dense forms as a GPU
    tensor is required, by the strided form as "a GPU fp16 tensor"; no output is no check."""
    o = torch.zeros(4, 64, dtype=torch.float16)
    ops._check_o(None, 4, 64, "w")
    with pytest.raises(ops.VQError, match="o must be a GPU tensor"):
        ops._check_o(o, 4, 64, "w")
    with pytest.raises(ops.VQError, match="o must be a GPU fp16 tensor"):
        ops._check_o(o, 4, 64, None, strided=True)
