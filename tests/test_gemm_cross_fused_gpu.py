"""vq_gemm_i8_cross_attn: cross_attn.q_linear's int8 GEMM with cross attention against the prompt's <= 128 keys in its
epilogue (q is never written).  att_o against the two launches it replaces - vq_gemm_i8 into a dense q, then vq_attn_fwd -
bit for bit: every tile count, k-tile count, weight width, bias and key count of the contract; score structures that take
and defer the rescale of the online softmax; an input that puts a swapped head or query block into a wrong row; every
refusal of the shape contract; and one STDiT and one PixArt block (hidden 288, 4 heads, 256 tokens) behind the route
switch."""
import functools
import itertools

import pytest
import torch

import attn_regimes as ar
from helpers import trace_ops

pytestmark = pytest.mark.gpu

D = 72
KEYS = (1, 63, 64, 65, 120, 128)
SHAPES = list(itertools.product((256, 512), (288, 576, 1152), (128, 256, 1152), (8, 4), (False, True)))


@functools.lru_cache(maxsize=None)
def _linear(M, N, K, w_bits, dev, x_scale=1.0):
    """q_linear's operands the way the model makes them: per-token 8-bit codes of a random activation, a min-max packed
    weight of ``w_bits`` and a bias.  Computed once per shape, never modified."""
    from viditq_amd import ops
    g = torch.Generator().manual_seed(M + 7 * N + 13 * K + w_bits)
    x = (torch.randn(1, M, K, generator=g) * x_scale).half().to(dev)
    W = (torch.randn(N, K, generator=g) * K ** -0.5).half().to(dev)
    delta, zp = ops.weight_minmax(W, w_bits)
    bias = (torch.randn(N, generator=g) * 0.3).float().to(dev)
    return ops.rowquant(x, n_bits=8), ops.pack_weight(W, delta, zp, w_bits), bias


@functools.lru_cache(maxsize=None)
def _prompt(H, lens, dev, seed=5):
    """K | V rows [sum(lens), 2 H D] of the samples' prompts, packed the way the model packs them, and their offsets."""
    g = torch.Generator().manual_seed(seed + H + sum(lens))
    kv = torch.randn(sum(lens), 2 * H * D, generator=g).half().to(dev)
    offs = torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int32, device=dev)
    return kv, offs


def _pair(ops, qa, pw, bias, kv, offs, n_seq, bound, scale=None):
    """The two launches: the dense q of vq_gemm_i8 and vq_attn_fwd on it."""
    M, N = qa.rows, pw.N
    H, Lq = N // D, M // n_seq
    q = ops.gemm_i8(qa, pw, bias=bias)
    o = torch.full((M, N), 7.0, dtype=torch.float16, device=q.device)
    ops.attn_fwd(q, kv, kv[:, N:], o, n_seq, Lq, bound, H, D, Lq * N, N, 0, kv.stride(0), Lq * N, N, kv_off=offs, scale=scale)
    return q, o


def _fused(ops, qa, pw, bias, kv, offs, n_seq, bound, scale=None):
    M, N = qa.rows, pw.N
    H, Lq = N // D, M // n_seq
    o = torch.full((M, N), -7.0, dtype=torch.float16, device=kv.device)
    return ops.gemm_i8_cross_attn(qa, pw, bias, kv, kv[:, N:], o, n_seq, Lq, bound, H, D, 0, kv.stride(0), Lq * N, N,
                                  kv_off=offs, scale=scale)


def _same(got, ref, what):
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        r, c = int(bad[0, 0]), int(bad[0, 1])
        raise AssertionError("%s: %d of %d elements differ, first at row %d column %d (head %d): %r vs %r" % (
            what, bad.shape[0], got.numel(), r, c, c // D, float(got[r, c]), float(ref[r, c])))
    assert bool(torch.isfinite(got).all()), what


@pytest.mark.parametrize("M,N,K,w_bits,with_bias", SHAPES, ids=["%dx%dx%d-w%d-%s" % (s[:4] + ("bias" if s[4] else "nobias",))
                                                              for s in SHAPES])
def test_fused_equals_gemm_then_cross_attention(ops, dev, M, N, K, w_bits, with_bias):
    """One sample of M tokens against every key count; M = 512 also as two samples with different key counts (one tile
    row each)."""
    qa, pw, bias = _linear(M, N, K, w_bits, dev)
    bias = bias if with_bias else None
    H = N // D
    runs = [(1, (L,)) for L in KEYS]
    if M == 512:
        runs += [(2, (120, 37)), (2, (1, 128)), (2, (64, 65))]
    for n_seq, lens in runs:
        kv, offs = _prompt(H, lens, dev)
        _, ref = _pair(ops, qa, pw, bias, kv, offs, n_seq, max(lens))
        got = _fused(ops, qa, pw, bias, kv, offs, n_seq, max(lens))
        _same(got, ref, "n_seq %d keys %r" % (n_seq, lens))
    # without offsets: Lk rows per sample, kv_seq_stride apart
    L = 120
    kv, _ = _prompt(H, (L,) * 2, dev)
    n_seq, Lq = (2, M // 2) if M == 512 else (1, M)
    q = ops.gemm_i8(qa, pw, bias=bias)
    ref = torch.empty_like(q)
    ops.attn_fwd(q, kv, kv[:, N:], ref, n_seq, Lq, L, H, D, Lq * N, N, L * kv.stride(0), kv.stride(0), Lq * N, N)
    got = ops.gemm_i8_cross_attn(qa, pw, bias, kv, kv[:, N:], torch.empty_like(q), n_seq, Lq, L, H, D, L * kv.stride(0),
                                 kv.stride(0), Lq * N, N)
    _same(got, ref, "dense K | V")
    # a bound above the samples' own counts (the model passes the longest prompt of the batch)
    kv, offs = _prompt(H, (37,), dev)
    _same(_fused(ops, qa, pw, bias, kv, offs, 1, 128), _pair(ops, qa, pw, bias, kv, offs, 1, 128)[1], "bound 128, 37 keys")


# ---------------------------------------------------------------------------------------------------- softmax edges
def _rescales(q, kv, N, lens, n_seq, scale):
    """From the dense q of the two-launch path: per (sample, head, 32-query block) the walk of the 32-key half tiles the
    kernels make - (number of blocks whose running maximum moves on a LATER half tile, i.e. with O already accumulated,
    number of late half tiles that lead by less than 8 and defer)."""
    M = q.shape[0]
    H, Lq = N // D, M // n_seq
    taken = deferred = 0
    off = 0
    for s in range(n_seq):
        L = lens[s]
        qs = q[s * Lq:(s + 1) * Lq].view(1, Lq, H, D).cpu()
        ks = kv[off:off + L, :N].reshape(1, L, H, D).cpu()
        off += L
        sc = ar.scores(qs, ks, scale, [L])[0]                      # [H, Lq, L], exp2 domain
        nh = (L + 31) // 32
        hm = torch.stack([sc[:, :, 32 * h:32 * h + 32].max(-1).values for h in range(nh)], -1)     # [H, Lq, nh]
        for h in range(H):
            for b in range(Lq // 32):
                run = None
                for t in range(nh):
                    m = hm[h, 32 * b:32 * b + 32, t]
                    if run is None:
                        run = m.clone()
                        continue
                    lead = m - run
                    if bool((lead > 8.0).any()):
                        taken += 1
                        run = torch.maximum(run, m)
                    elif bool((lead > 0).any()):
                        deferred += 1
    return taken, deferred


def _rank_one(M, N, K, dev, t, c):
    """Operands whose GEMM output is q[m, n] = t[m] c[n] exactly as fp32 products go: zero weight codes with zw = -1 and
    cs = 0 leave sx[m] sw[n] R[m]; sx = |t| 2^-10, R = sign(t) 2^10, sw = c."""
    from viditq_amd import ops
    Kp = ops.pad128(K)
    qa = ops.QAct(torch.zeros(M, Kp, dtype=torch.int8, device=dev), (t.abs() * 2.0 ** -10).float().to(dev),
                  torch.zeros(M, dtype=torch.int32, device=dev), (torch.sign(t) * 1024).int().to(dev), K, 8)
    pw = ops.PackedWeight(torch.zeros(N, Kp, dtype=torch.int8, device=dev), c.float().to(dev),
                          torch.full((N,), -1, dtype=torch.int32, device=dev), torch.zeros(N, dtype=torch.int32, device=dev),
                          N, K, Kp, 8)
    return qa, pw


def _profile_keys(H, L, prof, dev, seed=11):
    """Keys that are zero except for channel D - 1 of every head, which holds prof[j]; random V."""
    g = torch.Generator().manual_seed(seed)
    kv = torch.zeros(L, 2 * H * D)
    kv[:, H * D:] = torch.randn(L, H * D, generator=g)
    for h in range(H):
        kv[:, h * D + D - 1] = prof
    return kv.half().to(dev), torch.tensor([0, L], dtype=torch.int32, device=dev)


EDGES = ["rising_9", "rising_24", "rising_7", "falling_24", "second_image", "one_key", "all_equal", "random_large",
         "shifted"]


@pytest.mark.parametrize("edge", EDGES)
def test_softmax_edges_match_bit_for_bit(ops, dev, edge):
    """Score structures of tests/attn_regimes.py on the fused launch.  q = t[m] e_(D-1) per head (rank one, exact), so a
    query's scores are t[m] x the keys' profile: staircases over the 32-key half tiles that lead by more (rescale taken on
    late tiles, O already accumulated) or less (deferred) than 8 in the exp2 domain, rising for even and falling for odd
    queries; a maximum that first appears in the second 64-key image; one dominant key; all-equal scores; and the random
    GEMM's q scaled so that its scores have a standard deviation of about 17, and shifted by +-300 on one channel."""
    M, N, K, L = 256, 288, 128, 64 if edge == "rising_7" else 120      # (over four half tiles a lead of 7 adds up to 14)
    H, scale = N // D, D ** -0.5
    u = scale * ar.LOG2E
    if edge in ("random_large", "shifted"):
        qa, pw, bias = _linear(M, N, K, 8, dev, x_scale=12.0)
        kv, offs = _prompt(H, (L,), dev)
        if edge == "shifted":
            # +-300 (exp2 domain) on every score of a row through channel D - 1: bias a, keys a, sign by the row's head
            a = (300.0 / u) ** 0.5
            kv = kv.clone()
            bias = bias.clone()
            for h in range(H):
                kv[:, h * D + D - 1] = a
                bias[h * D + D - 1] = a if h % 2 == 0 else -a     # (the GEMM's own term of that channel is small beside a)
    else:
        t = torch.ones(M)
        t[1::2] = -1.0                                             # odd queries see the mirrored profile
        c = torch.zeros(N)
        c[D - 1::D] = 4.0
        j = torch.arange(L)
        step = {"rising_9": 9.0, "rising_24": 24.0, "rising_7": 7.0, "falling_24": -24.0}.get(edge)
        if step is not None:
            prof = (j // 32).double() * step
        elif edge == "second_image":
            prof = (j >= 64).double() * 40.0 + (j == 100).double() * 30.0
        elif edge == "one_key":
            prof = (j == 77).double() * 250.0
        else:
            prof = torch.zeros(L, dtype=torch.float64)
        qa, pw = _rank_one(M, N, K, dev, t, c)
        bias = None
        kv, offs = _profile_keys(H, L, (prof / (4.0 * u)).float(), dev)
    q, ref = _pair(ops, qa, pw, bias, kv, offs, 1, L)
    got = _fused(ops, qa, pw, bias, kv, offs, 1, L)
    taken, deferred = _rescales(q, kv, N, (L,), 1, scale)
    print("%s: rescale taken on a late half tile in %d blocks, deferred on %d half tiles" % (edge, taken, deferred))
    if edge in ("rising_9", "rising_24", "falling_24", "second_image", "one_key", "random_large"):
        assert taken > 0, "the rescale branch must be taken with O accumulated"
    if edge == "rising_7":
        assert deferred > 0 and taken == 0, "a lead below 8 defers"
    if edge == "all_equal":
        assert taken == 0 and deferred == 0
        v = kv[:, N:].float().view(L, H, D)
        assert torch.allclose(ref.float().view(M, H, D), v.mean(0)[None].expand(M, H, D), atol=2e-3), "uniform softmax"
    _same(got, ref, edge)


def test_heads_and_query_blocks_land_in_their_rows(ops, dev):
    """q constant per (token, head) - q[m, h, :] = t[m] c[h], all products distinct - against keys of all ones: a token's
    softmax over the prompt depends on (token, head) alone, so an output row or head segment taken from another unit
    differs.  Two tile rows and two tile columns (M = 512, N = 576), two samples."""
    M, N, K, lens = 512, 576, 128, (120, 77)
    H = N // D
    t = 0.25 + torch.arange(M).float() / 256.0
    c = (1.0 + torch.arange(H).float() * 0.37).repeat_interleave(D) / D
    qa, pw = _rank_one(M, N, K, dev, t, c)
    g = torch.Generator().manual_seed(3)
    kv = torch.zeros(sum(lens), 2 * N)
    kv[:, :N] = (torch.arange(sum(lens)).float() % 13 - 6.0)[:, None] * 0.5      # one score per key, the same for every head
    kv[:, N:] = torch.randn(sum(lens), N, generator=g)
    kv = kv.half().to(dev)
    offs = torch.tensor([0, lens[0], sum(lens)], dtype=torch.int32, device=dev)
    q, ref = _pair(ops, qa, pw, None, kv, offs, 2, max(lens))
    qh = q.view(M, H, D)
    assert bool((qh == qh[:, :, :1]).all()), "constant per (token, head)"
    assert all(qh[:, h, 0].unique().numel() == M for h in range(H)) and all(
        qh[m, :, 0].unique().numel() == H for m in (0, 255, 256, 511)), "distinct over the tokens of a head and over the heads"
    got = _fused(ops, qa, pw, None, kv, offs, 2, max(lens))
    _same(got, ref, "layout")
    # the rows themselves differ from one 32-query block and from one head to the next: a swap could not hide
    r = ref.view(M, H, D).float()
    assert not torch.equal(r[0:32], r[32:64]) and not torch.equal(r[:, 0], r[:, 1]) and not torch.equal(r[0:256], r[256:512])


# ---------------------------------------------------------------------------------------------------- refusals
def test_every_clause_of_the_shape_contract_refuses(ops, dev):
    """VQ_ESHAPE (-2) and an untouched att_o for: M = 255, N = 360 (five heads), a bound of 129 keys, a pointer off 16 bytes,
    and a 256-row tile that spans two samples."""
    from viditq_amd import _lib
    lib = _lib.load()
    M, N, K = 512, 288, 128
    qa, pw, bias = _linear(M, N, K, 8, dev)
    kv, offs = _prompt(N // D, (120, 37), dev)
    kv5, _ = _prompt(5, (120, 37), dev)
    o = torch.full((M + 1, 360), 3.0, dtype=torch.float16, device=dev)
    p = lambda t: t.data_ptr()
    st = torch.cuda.current_stream().cuda_stream

    def call(M_=M, N_=N, n_seq=2, Lq=256, Lk=120, H=N // D, k=kv, ko=N, obuf=p(o), xq=p(qa.xq), ldo=N):
        return lib.vq_gemm_i8_cross_attn(xq, p(qa.sx), p(qa.zx), p(qa.R), p(pw.wq), p(pw.sw), p(pw.zw), p(pw.cs), p(bias),
                                         p(k), p(k) + 2 * ko, obuf, M_, N_, K, qa.Kp, 8, n_seq, Lq, Lk, H, D, 0, k.stride(0),
                                         Lq * ldo, ldo, p(offs), D ** -0.5, st)
    assert call(M_=255, n_seq=1, Lq=255) == -2
    assert call(N_=360, H=5, k=kv5, ko=360, ldo=360) == -2
    assert call(Lk=129) == -2
    assert call(obuf=p(o) + 2) == -2 and call(xq=p(qa.xq) + 1) == -2 and call(ko=N + 1) == -2
    assert call(n_seq=2, Lq=256, M_=768) == -2                     # M != n_seq * Lq
    assert call(n_seq=4, Lq=128) == -2                             # tiles of 256 rows span two samples
    assert call(n_seq=1, Lq=512, H=8) == -2                        # N != H * D
    torch.cuda.synchronize()
    assert bool((o == 3.0).all()), "a refused call writes nothing"
    with pytest.raises(ops.VQError):
        ops.gemm_i8_cross_attn(qa, pw, bias, kv, kv[:, N:], o[:M, :N].contiguous(), 2, 256, 129, N // D, D, 0, kv.stride(0),
                               256 * N, N, kv_off=offs)
    assert call() == 0                                             # the same call, within the contract
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- model level
def _tiny_stdit(dev):
    from viditq_amd import synth
    from viditq_amd.config import loads_yaml
    m = synth.build_stdit(dev, depth=1, hidden_size=288, num_heads=4, input_size=(4, 16, 16), model_max_length=24,
                          caption_channels=64)
    qnn = synth.quantize_model(m, loads_yaml(synth.W8A8_DYNAMIC))
    assert all(b.fused_ok() for b in qnn.model.blocks)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 4, 4, 16, 16, generator=g).to(dev)
    y = (torch.randn(1, 1, 24, 64, generator=g) * 0.5).half().to(dev)
    mask = torch.zeros(1, 24, dtype=torch.int64, device=dev)
    mask[0, :19] = 1
    return lambda: qnn(x, torch.tensor([500], device=dev), y, mask=mask)


def _tiny_pixart(dev):
    from viditq_amd import synth
    from viditq_amd.config import to_config
    from viditq_amd.qdiff.models import QuantModel
    from viditq_amd.t2i.pixart import PixArtMS
    torch.manual_seed(0)
    m = PixArtMS(input_size=32, hidden_size=288, depth=1, num_heads=4, caption_channels=64, model_max_length=24,
                 dtype=torch.float16)
    synth.redraw_zero_init(m, 1)
    m = m.half().to(dev).eval()
    wq = to_config(dict(n_bits=8, per_group="channel", channel_dim=0, scale_method="min_max", round_mode="nearest"))
    aq = to_config(dict(n_bits=8, per_group="token", scale_method="min_max", round_mode="nearest_ste", running_stat=False,
                        dynamic=True, sym=False, n_spatial_token=256, n_temporal_token=1, n_prompt=24,
                        smooth_quant=dict(enable=False)))
    qnn = QuantModel(m, wq, aq, model_type="pixart")
    qnn.set_module_name_for_quantizer(qnn.model)
    qnn.fp_layer_list = ["x_embedder", "t_embedder", "t_block", "y_embedder", "csize_embedder", "ar_embedder"]
    synth.init_weight_quantizers(qnn)
    qnn.set_quant_state(True, True)
    assert all(b.fused_ok() for b in qnn.model.blocks)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 4, 32, 32, generator=g).to(dev)
    y = (torch.randn(2, 1, 24, 64, generator=g) * 0.5).half().to(dev)
    mask = torch.zeros(2, 24, dtype=torch.int64, device=dev)
    mask[0, :24] = 1
    mask[1, :7] = 1
    return lambda: qnn(x, torch.tensor([820, 820], device=dev), y, mask=mask)


@pytest.mark.parametrize("model", ["stdit", "pixart"])
def test_block_output_is_the_same_behind_the_switch(ops, dev, model, monkeypatch):
    """One block of hidden 288 / 4 heads over 256 tokens: with the route on, the cross stage makes ONE gemm_i8_cross_attn call
    and no attn_fwd call; the model's output equals the route-off output bit for bit."""
    from viditq_amd.t2v import stdit
    run = (_tiny_stdit if model == "stdit" else _tiny_pixart)(dev)
    monkeypatch.setattr(stdit, "_CROSS_Q_FUSED_ROUND", 1)            # one or two tiles: the shape contract alone decides here
    outs, calls = {}, {}
    for on in (False, True):
        monkeypatch.setattr(stdit, "_CROSS_Q_FUSED", on)
        run()                                                      # packing and caches
        with trace_ops() as tr:
            outs[on] = run().clone()
        torch.cuda.synchronize()
        calls[on] = [c[0] for c in tr]
    n_cross_off = sum(1 for c in calls[False] if c == "attn_fwd")
    assert calls[False].count("gemm_i8_cross_attn") == 0 and n_cross_off >= 1
    assert calls[True].count("gemm_i8_cross_attn") == 1
    assert calls[True].count("attn_fwd") == n_cross_off - 1, "the cross attention launch is gone"
    assert calls[True].count("gemm_i8") == calls[False].count("gemm_i8") - 1, "and q_linear's GEMM with it"
    assert bool(torch.isfinite(outs[True]).all())
    assert torch.equal(outs[True], outs[False])
