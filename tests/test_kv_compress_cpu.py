"""Host side of the key / value compression route: ops.kv_compress_ok's truth table, the wrapper's refusal of CPU tensors and
AttentionKVCompress's route predicate on CPU tensors (the torch sequence, the library never loaded)."""
import pytest
import torch


@pytest.mark.parametrize("args,ok", [
    ((1152, 128, 128, 2, "conv", 3456), True), ((1152, 64, 64, 4, "uniform", 3456), True), ((64, 4, 6, 2, "ave", 200), True),
    ((2048, 8, 4, 4, "conv", 6144), True), ((64, 3, 4, 2, "uniform_every", 192), True),      # 12 tokens, every 2nd
    ((64, 6, 6, 3, "conv", 192), False), ((64, 5, 4, 2, "conv", 192), False), ((64, 4, 5, 2, "ave", 192), False),
    ((64, 3, 3, 2, "uniform_every", 192), False), ((60, 4, 4, 2, "conv", 192), False), ((2056, 4, 4, 2, "conv", 6168), False),
    ((64, 4, 4, 2, "conv", 184), False), ((64, 4, 4, 2, "conv", 196), False), ((64, 4, 4, 2, None, 192), False),
    ((64, 4, 4, 2, "nearest", 192), False), ((64, 4, 4, 1, "conv", 192), False)])
def test_kv_compress_ok_truth_table(args, ok):
    import viditq_amd  # noqa: F401
    from viditq_amd import ops
    assert ops.kv_compress_ok(*args) is ok


def test_cpu_tensors_fall_back_and_never_reach_the_library(monkeypatch):
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib, ops
    from viditq_amd.t2i import pixart

    def reached(*a, **k):
        raise AssertionError("a CPU tensor got as far as the library")
    monkeypatch.setattr(_lib, "load", reached)
    qkv = torch.zeros(16, 192, dtype=torch.float16)
    with pytest.raises(ops.VQError):
        ops.kv_compress(qkv, 1, 4, 4, 64, 2, "uniform")
    assert pixart._KV_COMPRESS_HIP is False                           # a route that moves results: default off
    monkeypatch.setattr(pixart, "_KV_COMPRESS_HIP", True)
    attn = pixart.AttentionKVCompress(64, num_heads=4, sampling="conv", sr_ratio=2, qk_norm=True)
    assert not attn.kv_compress_hip(qkv, 16, 4, 4)                    # a CPU buffer
    meta = torch.empty(16, 192, dtype=torch.float16, device="meta")
    assert not attn.kv_compress_hip(meta.float(), 16, 4, 4) and not attn.kv_compress_hip(qkv, 16, 2, 4)
    monkeypatch.setattr(ops, "attn_fwd", lambda q, k, v, o, *a, **kw: o.zero_())   # (the HIP attention needs a GPU)
    monkeypatch.setattr(ops, "kv_compress", reached)
    assert attn.attend(qkv, 1, 16, (4, 4)).shape == (16, 64)          # the torch sequence ran
