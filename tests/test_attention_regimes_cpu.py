"""CPU checks behind test_attention_softmax_gpu.py: every case reaches the kernel it names (vq_attn_fwd_route with dummy
pointers, no GPU), every kernel of the table is covered under R1, R2 and R3, and the input builders of attn_regimes.py
build what their names say (gaps, per-tile leads, row shifts; fp64 on the fp16 tensors)."""
import ctypes
import math

import pytest
import torch

import attn_regimes as ar

CASES = ar.cases()
IDS = ar.kernel_ids()
# head dims of the kernel table
TABLE_DIMS = {"VQ_ATTN_K_CROSS32_2": {16, 32, 64, 72}, "VQ_ATTN_K_CROSS32_3": {64, 72}, "VQ_ATTN_K_CROSS32_4": {64, 72},
              "VQ_ATTN_K_CROSS32_5": {64, 72}, "VQ_ATTN_K_CROSS_REG": {72}, "VQ_ATTN_K_FWD8_NW8": {72}}


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from viditq_amd import _lib as L
    return L.load()


def _route(lib, case, ptr=1 << 20):
    a = ar.fwd_layout(case)
    p = ctypes.c_void_p(ptr)
    off = p if a["offs"] is not None else None
    return lib.vq_attn_fwd_route(p, p, p, p, a["n_seq"], a["Lq"], a["Lk"], a["H"], a["D"], a["q_seq"], a["q_tok"],
                                 a["kv_seq"], a["kv_tok"], a["o_seq"], a["o_tok"], off, case["scale"], None)


def test_every_case_reaches_the_kernel_it_names():
    lib = _lib()
    for c in CASES:
        if c["kernel"].startswith("VQ_ATTN_K_"):
            assert _route(lib, c) == IDS[c["kernel"]], c["id"]
        else:
            assert ar.temporal_route(c) == c["kernel"], c["id"]


def test_every_kernel_of_the_table_is_covered_by_each_regime():
    kernels = ar.FWD_KERNELS + ar.TEMPORAL_KERNELS
    assert set(ar.FWD_KERNELS) == set(IDS)
    for reg in ("R1", "R2", "R3"):
        for kern in kernels:
            dims = {c["D"] for c in CASES if c["kernel"] == kern and c["regime"][0] == reg}
            assert dims == TABLE_DIMS.get(kern, {16, 32, 64, 72}), (reg, kern, dims)
    # R2: rising and falling, deferred (lead < 8) and taken (lead > 8) rescales, tiles of 64, 32 and 16 keys
    r2 = [c["regime"] for c in CASES if c["regime"][0] == "R2"]
    assert {r[3] for r in r2} == {False, True} and {r[2] for r in r2} == {7.0, 9.0, 24.0} and {16, 32, 64} <= {r[1] for r in r2}
    assert {c["regime"][1] for c in CASES if c["regime"][0] == "R3"} == {150.0, 300.0}
    # R4: the scale argument at 1.0 and 0.02 under R1 and R2, every kernel family
    for reg in ("R1", "R2"):
        for s in (1.0, 0.02):
            fam = {c["kernel"] for c in CASES if c["regime"][0] == reg and c["scale"] == s}
            assert len(fam) >= 8, (reg, s, fam)
    # T of the long temporal kernel: 17, 33, 64 and one T <= 16
    assert {c["shape"]["T"] for c in CASES if c["kernel"] == "attn_temporal_long"} >= {17, 33, 64, 12}
    assert len({c["id"] for c in CASES}) == len(CASES)


def test_the_route_hook_agrees_with_the_documented_dispatch_edges():
    """Edges of the table: the query / key bounds and the byte extent that switch kernels."""
    lib = _lib()

    def route(n, Lq, Lk, H, D, kv_off=False, kv_tok=None):
        c = dict(D=D, scale=D ** -0.5, shape=dict(n=n, Lq=Lq, lens=[Lk] * n, H=H, kv_off=kv_off))
        if kv_tok:
            c["shape"]["kv_stride"] = kv_tok
        return _route(lib, c)
    assert route(1, 95, 300, 2, 64) == IDS["VQ_ATTN_K_FWD"]
    assert route(1, 96, 300, 2, 64) == IDS["VQ_ATTN_K_FWD8_NW4"]
    assert route(1, 191, 300, 2, 64) == IDS["VQ_ATTN_K_FWD8_NW4"]
    assert route(1, 192, 300, 2, 64) == IDS["VQ_ATTN_K_FWD32D"]
    assert route(1, 192, 128, 2, 64) == IDS["VQ_ATTN_K_FWD"]
    assert route(1, 256, 128, 2, 64) == IDS["VQ_ATTN_K_CROSS32_2"]
    assert route(1, 2048, 2048, 2, 64) == IDS["VQ_ATTN_K_FWD64D"]
    assert route(1, 2047, 2048, 2, 64) == IDS["VQ_ATTN_K_FWD32D"]
    assert route(1, 2048, 2048, 1, 72, kv_tok=1 << 19) == IDS["VQ_ATTN_K_FWD8_NW8"]
    assert route(1, 2048, 2048, 1, 72, kv_tok=(1 << 19) - 8) == IDS["VQ_ATTN_K_FWD64D"]
    assert route(1, 100, 2048, 1, 72, kv_tok=1 << 19) == IDS["VQ_ATTN_K_FWD8_NW4"]
    assert route(1, 100, 120, 8, 72) == IDS["VQ_ATTN_K_CROSS_REG"]
    assert route(1, 63, 120, 8, 72) == IDS["VQ_ATTN_K_FWD"]
    assert route(1, 300, 129, 2, 72, kv_off=True) == IDS["VQ_ATTN_K_CROSS32_3"]
    assert route(1, 300, 321, 2, 72, kv_off=True) == IDS["VQ_ATTN_K_FWD"]
    assert route(1, 300, 300, 2, 32, kv_off=True) == IDS["VQ_ATTN_K_FWD"]          # 3-5 tile images: D >= 64 only
    assert route(1, 300, 129, 2, 77) == -2                                        # unsupported head dim


# ----------------------------------------------------------------------------- builders
@pytest.mark.parametrize("D,Lq,lens,scale", [(16, 300, [2100], None), (72, 200, [333, 65], None), (32, 64, [17], 1.0),
                                             (64, 128, [1000], 0.02), (72, 64, [64], None)])
def test_r1_rows_are_one_hot(D, Lq, lens, scale):
    scale = D ** -0.5 if scale is None else scale
    H = 2
    q, k, v, hot = ar.r1(len(lens), Lq, lens, H, D, scale, seed=D + Lq)
    g = ar.gaps(q, k, hot, scale, lens)
    assert float((g >= ar.R1_GAP).double().mean()) >= 0.9
    s = ar.scores(q, k, scale, lens)
    assert float(s[torch.isfinite(s)].abs().max()) <= 300.0
    for i, L in enumerate(lens):                 # the sweep of hot keys over a sequence with Lq >= its length
        used = set(hot[i, :, 0].tolist())
        assert 0 in used and L - 1 in used and set(range(64 * (L // 64), L)) <= used
        if Lq >= len(ar.hot_sweep(L)):
            assert {j % 64 for j in used} == set(range(min(64, L)))
        assert all(0 <= j < L for j in used)
    assert torch.all(v[0, lens[0]:] == 0)


@pytest.mark.parametrize("step,lead,falling", [(64, 7.0, False), (64, 9.0, True), (32, 24.0, False), (16, 9.0, False),
                                               (64, 24.0, True)])
@pytest.mark.parametrize("D,scale", [(72, None), (16, None), (64, 1.0), (32, 0.02)])
def test_r2_tiles_lead_by_the_stated_step(step, lead, falling, D, scale):
    scale = D ** -0.5 if scale is None else scale
    Lk = 4160
    q, k, _ = ar.r2(1, 8, [Lk], 1, D, scale, seed=5, step=step, lead=lead, falling=falling)
    s = ar.scores(q, k, scale, [Lk])[0, 0]                          # [8, Lk]
    assert float(s.max()) <= 255.0 and float(s.min()) >= -5.0
    tmax = s.reshape(8, Lk // step, step).max(-1).values             # tile maxima
    P = int(ar.R2_MAX // lead) + 1
    assert Lk // step > P                                            # the sawtooth wraps at least once
    for t in range(1, P):
        run = tmax[:, :t].max(-1).values
        d = tmax[:, t] - run
        if falling:
            assert bool((d < -lead + 0.6).all()), t                  # later tiles trail: no rescale
        else:
            assert bool(((d - lead).abs() < 0.6).all()), t           # every tile of the first tooth leads by `lead`
            assert bool(((d - 8.0).abs() > 0.4).all())               # ... clearly on one side of the rescale threshold


@pytest.mark.parametrize("shift", [150.0, 300.0])
@pytest.mark.parametrize("D,lens", [(72, [333]), (16, [100, 37])])
def test_r3_rows_shift_by_a_common_constant(shift, D, lens):
    scale = D ** -0.5
    Lq = 64
    q, k, v = ar.r3(len(lens), Lq, lens, 2, D, scale, seed=9, shift=shift)
    s = ar.scores(q, k, scale, lens)
    q0 = q.clone()
    q0[..., ar.DSTAR] = 0
    base = ar.scores(q0, k, scale, lens)
    for i, L in enumerate(lens):
        d = (s - base)[i, :, :, :L]                                   # [H, Lq, L]
        assert float((d - d[..., :1]).abs().max()) < 1e-9             # one constant per row (fp64 sums of exact products)
        sign = torch.where(torch.arange(Lq) % 2 == 0, 1.0, -1.0).double()
        assert bool(((d[..., 0] - sign * shift).abs() < 1.0).all())
        assert float(base[i, :, :, :L].abs().max()) < 30.0
        assert bool((torch.isinf(s[i, :, :, L:])).all())
    assert math.isclose(float(s[torch.isfinite(s)].abs().max()), shift, rel_tol=0.1)
