"""Every quantizer kernel at rounding ties, grid edges and fp16 extremes (quant_rows.py), against the oracle's
clamp(round_half_even(RN(x / delta)) + zp, 0, qmax) - bit for bit.

Random N(0, s^2) rows never hold an exact tie, never put -min / delta on x.5, never straddle the 1e-6 eps threshold and
leave the position of the row extremum to chance; there the shortcuts of csrc/vq_common.h (vq_row_grid's Markstein delta,
1-ulp reciprocal and guarded zero point; rq_round_group's packed fma with one tie test per group; rq_div_rcp) cannot be
told from the reference arithmetic.  Here:
  Q1  every value but the row's min / max is an exact tie on a 2^-k grid, zero points odd, even, 0 and qmax;
  Q2  the same rows behind s = 1 + j 2^-23: quotients 1e-6 .. 1e-3 from a tie on both sides (below the claimed error of
      the product form, between it and the 1e-4 guard, past the guard);
  Q3  max = -min over the fp16 magnitudes: -min / delta = 127.5 (31.5);
  Q4  [0, m] rows with delta on both sides of 1e-6 (and, behind a smoothing vector, AT 1e-6 and one ulp to either side);
  Q5  +-65504, subnormals, -0.0;  Q6  the extremum at chosen lanes.
There is no tolerance and no excluded share of elements where the oracle is the reference: codes, delta, zero point,
row term R, zero padding and the status word are compared exactly.  Rows the oracle would eps-fill run one per launch
and must raise VQ_ST_EPSFILL (the kernels leave the refill to vq_epsfill_fixup, so no codes are compared there);
test_quant_rows_cpu.py shows that no bit-exact launch holds such a row.

vq_gelu_rowquant and vq_ln_modulate_rowquant compute their quantizer input on the GPU, so exact ties cannot be placed
here; they run Q3 / Q5 / Q6 under the relations (and bounds) of test_kernels_gpu.py.  Their quantizer input itself is
pinned elsewhere: the GELU value at every call site over all finite fp16 inputs by test_gelu_rowquant_exact_gpu.py
(gelu_cases.py), LayerNorm + modulate by test_ln_modulate_exact_gpu.py (ln_cases.py)."""
import os
import subprocess
import sys

import pytest
import torch

import quant_rows as qr
from oracle import fakequant as fq

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("xq", "sx", "zx", "R")


def _first_diff(got, want, what):
    bad = (got != want).nonzero()
    i = tuple(bad[0].tolist())
    return "%s: %d differ, first at %s: oracle %s, kernel %s" % (what, bad.shape[0], i, want[i].item(), got[i].item())


def _check_exact(qa, st, x, n_bits, s, what, delta=None, zp=None):
    """qa against the oracle's quantizer of x [B, n, C] (behind s; on the static grid delta / zp when given)."""
    B, n, C = x.shape
    xin = qr.smoothed(x, s)
    if delta is None:
        codes, _, d, z, eps = fq.dyn_act_quant(xin, n_bits)
        assert not eps, what
        d, z = d.reshape(1, n).expand(B, n), z.reshape(1, n).expand(B, n)
    else:
        d = delta.reshape(1, -1).expand(B, n)
        z = zp.reshape(1, -1).expand(B, n)
        codes, _ = fq.static_act_quant(xin, d[0].reshape(1, n, 1), z[0].reshape(1, n, 1), n_bits)
    cx = 128 if n_bits == 8 else 0
    codes = codes.int()
    got = qa.xq[:, :C].cpu().int().reshape(B, n, C) + cx
    assert torch.equal(got, codes), _first_diff(got, codes, what + " codes")
    assert bool((qa.xq[:, C:] == 0).all()), what + " padding"
    sx = qa.sx.cpu().reshape(B, n)
    assert torch.equal(sx, d.contiguous()), _first_diff(sx, d, what + " delta")
    zx = z.int() - cx
    assert torch.equal(qa.zx.cpu().reshape(B, n), zx), _first_diff(qa.zx.cpu().reshape(B, n), zx, what + " zx")
    if qa.zpf is not None:
        assert torch.equal(qa.zpf.cpu().reshape(B, n), z.contiguous()), what + " zpf"
    R = (codes - cx).sum(-1) - C * zx
    assert torch.equal(qa.R.cpu().reshape(B, n), R), _first_diff(qa.R.cpu().reshape(B, n), R, what + " R")
    if st is not None:
        assert int(st.item()) == 0, what + " status"


def _dynamic(ops, dev, B, C, n_bits, launch, s=None, fixed=False, small=True, ulp=False):
    """One route: the exact launch (every family, an odd row count that fills many workgroups), 131 and 257 rows thinned
    from it, 65 rows (the first count the LDS-staged smooth kernel takes) and 3 rows (one full pair and an odd tail: the
    upper half-wave or the partner wave re-does the last row and must write nothing), and the flagged launches.
    ``launch(x_dev, status) -> [(QAct, s or None), ...]``."""
    exact, flagged, names = qr.launch_sets(B, C, n_bits, s=s, q3_stride=7 if (B, C) == (1, 1152) else 49, fixed=fixed,
                                           ulp=ulp)
    sets = [exact] + ([qr.thin(exact, 131), qr.thin(exact, 257)] if small else []) + [qr.thin(exact, 65), qr.thin(exact, 3)]
    for x in sets:
        st = ops.new_status(dev)
        for j, (qa, sj) in enumerate(launch(x.to(dev), st)):
            _check_exact(qa, st, x, n_bits, sj, "B%d C%d b%d n%d out%d" % (B, C, n_bits, x.shape[1], j))
    for i, x in enumerate(flagged):
        st = ops.new_status(dev)
        launch(x.to(dev), st)
        assert fq.dyn_act_quant(qr.smoothed(x, s), n_bits)[4]
        assert int(st.item()) == 1, "B%d C%d b%d flagged launch %d: status %d" % (B, C, n_bits, i, int(st.item()))


# ----------------------------------------------------------------------------- un-smoothed dynamic quantizers
# shape -> kernel (vq_rowquant's dispatch):
#   B = 3, C = 64 / 96           rowquant_kernel (generic, IEEE division: vq_minmax_to_params + vq_code)
#   B = 1, C = 64 / 96 / 320     rowquant_fast_kernel<1>            B = 1, C = 4608   rowquant_fast_kernel<9>
#   B = 1, C = 768 .. 1280       rowquant_half_kernel (half-wave rows)
#   B = 2, C = 768 .. 1280       rowquant_half_kernel<.., PAIR>     B = 2, C = 4608   rowquant_fast_kernel<9, .., PAIR>
#   B = 2, C = 96                rowquant_fast_kernel<1, .., PAIR>
# (rowquant_split_kernel - a C = 4608 row over two partner waves - is built behind GELU only: see the GELU test below)
#   B = 1 / 2, C = 1408          rowquant_fast_kernel<3> / <3, .., PAIR>
PLAIN = [(3, 64), (3, 96), (1, 64), (1, 96), (1, 320), (1, 768), (1, 1024), (1, 1152), (1, 1280), (1, 4608), (2, 96),
         (2, 1152), (2, 768), (2, 4608), (2, 1024), (2, 1280), (1, 1408), (2, 1408)]


@pytest.mark.parametrize("n_bits", [8, 6])
@pytest.mark.parametrize("B,C", PLAIN)
def test_rowquant_edges(ops, dev, B, C, n_bits):
    _dynamic(ops, dev, B, C, n_bits, lambda x, st: [(ops.rowquant(x, n_bits=n_bits, status=st, want_zp=True), None)])


# ----------------------------------------------------------------------------- smoothed dynamic quantizers
def _svecs(C, dev, n_bits):
    """(s, s on the GPU, fixed): the Q2 vector (near ties; Q1 rows built with their min / max on its s = 1 channels) and a
    wide one whose launches also hold the q4u() rows (delta = 1e-6 to the ulp behind three of its channels)."""
    g = torch.Generator().manual_seed(C)
    out = [(qr.q2_smooth(C), True), (qr.q4u_vector(torch.exp(torch.randn(C, generator=g) * 0.7).float(), n_bits), False)]
    return [(s, s.to(dev), fixed) for s, fixed in out]


def _smooth_one_output(ops, dev):
    """B = 1, one smoothed output, C = 768 .. 1280: smooth_rowquant_multi_kernel<.., NOUT = 1> (vectors in LDS), or - in a
    process started with VQ_RQ_SM1=0 - smooth_rowquant_half_kernel (vectors in registers)."""
    for C in (1152, 768, 1024, 1280):
        for n_bits in (8, 6):
            for s, sd, fixed in _svecs(C, dev, n_bits):
                assert ops.smooth_rcp(sd) is not None
                _dynamic(ops, dev, 1, C, n_bits, lambda x, st: [(ops.rowquant(x, n_bits=n_bits, s=sd, status=st), s)],
                         s=s, fixed=fixed, small=C == 1152, ulp=not fixed)


def test_smoothed_one_output_vectors_in_lds_edges(ops, dev):
    _smooth_one_output(ops, dev)


def test_smoothed_one_output_vectors_in_registers_edges(ops, dev):
    """The same checks in a child process whose library reads VQ_RQ_SM1=0 (the switch is read once per process)."""
    code = ("import sys, torch; sys.path.insert(0, %r); sys.path.insert(0, %r); import viditq_amd; from viditq_amd import ops; "
            "import test_quantizer_edges_gpu as t\n"
            "with torch.no_grad():\n"
            "    t._smooth_one_output(ops, torch.device('cuda:0'))\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, VQ_RQ_SM1="0"), capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]


# B = 1, C = 4608 (n_tok >= 64)  rowquant_smooth_lds_kernel; with the zero point output or under 64 rows
#                                rowquant_fast_kernel<9, HAS_S> (reciprocal form from global memory)
# B = 2, C = 1152                smooth_rowquant_half_kernel<.., PAIR>      B = 2, C = 4608   rowquant_smooth_lds_kernel<.., PAIR>
# C = 1544 (Kp = 1664)           the same two LDS-staged kernels with a masked last chunk and pad columns [C, Kp) to zero
# fast_div=False                 the same kernels' IEEE-division branch (B = 1) / rowquant_kernel (B = 2)
@pytest.mark.parametrize("n_bits", [8, 6])
@pytest.mark.parametrize("B,C", [(1, 4608), (2, 1152), (2, 4608), (1, 1152), (1, 1544), (2, 1544), (2, 768)])
def test_smoothed_rowquant_edges(ops, dev, B, C, n_bits):
    for s, sd, fixed in _svecs(C, dev, n_bits):
        assert ops.smooth_rcp(sd) is not None

        def launch(x, st):
            outs = [(ops.rowquant(x, n_bits=n_bits, s=sd, status=st, fast_div=False), s)]
            if (B, C) != (1, 1152):                      # (B = 1, C = 1152 with the reciprocal: the two tests above)
                outs.append((ops.rowquant(x, n_bits=n_bits, s=sd, status=st), s))
            if B == 1:                                   # with zpf: rowquant_fast_kernel<.., HAS_S>, reciprocal form
                outs.append((ops.rowquant(x, n_bits=n_bits, s=sd, status=st, want_zp=True), s))
            return outs
        _dynamic(ops, dev, B, C, n_bits, launch, s=s, fixed=fixed, ulp=not fixed)


@pytest.mark.parametrize("n_bits", [8, 6])
@pytest.mark.parametrize("G", [2, 3])
def test_smoothed_outputs_of_one_pass_edges(ops, dev, G, n_bits):
    """smooth_rowquant_multi_kernel<.., NOUT = 2 / 3>: the Q2 vector, the same vector with its perturbations mirrored
    (every near tie approached from the other side) and a wide one, from one pass over the rows."""
    C = 1152
    s0 = qr.q2_smooth(C)
    vec = [s0, (2.0 - s0.double()).float(), torch.exp(torch.randn(C, generator=torch.Generator().manual_seed(G)) * 0.7).float()]
    vec = vec[:2] if G == 2 else vec
    dvec = [v.to(dev) for v in vec]
    for v in dvec:
        assert ops.smooth_rcp(v) is not None
    # rows clean behind every vector of the launch: select with each in turn
    exact = qr.launch_sets(1, C, n_bits, s=s0, q3_stride=49, fixed=True)[0]
    for v in vec:
        exact = exact[:, qr.split_eps(exact, n_bits, v)[0]]
    for x in (exact, qr.thin(exact, 131)):
        st = ops.new_status(dev)
        outs = ops.rowquant_multi(x.to(dev), dvec, n_bits=n_bits, status=st)
        for j, (qa, v) in enumerate(zip(outs, vec)):
            _check_exact(qa, st, x, n_bits, v, "multi%d out%d b%d n%d" % (G, j, n_bits, x.shape[1]))
    flagged = qr.launch_sets(1, C, n_bits, s=s0, q3_stride=49, fixed=True)[1]
    for x in flagged[:3]:
        st = ops.new_status(dev)
        ops.rowquant_multi(x.to(dev), dvec, n_bits=n_bits, status=st)
        assert int(st.item()) == 1


# ----------------------------------------------------------------------------- static grids
@pytest.mark.parametrize("n_bits", [8, 6])
@pytest.mark.parametrize("per_token", [True, False])
@pytest.mark.parametrize("B,n_tok,C", [(2, 37, 96), (1, 131, 1152), (1, 257, 4608)])
def test_static_grid_edges(ops, dev, B, n_tok, C, per_token, n_bits):
    """rowquant_kernel with delta / zp given (1 or n_tok entries), and fq_apply_kernel: Q1 ties on the calibrated grid plus
    values beyond both ends (both clamps act)."""
    x, delta, zp = qr.static_rows(B, n_tok, C, n_bits, per_token)
    qa = ops.rowquant(x.to(dev), n_bits=n_bits, delta=delta.to(dev), zp=zp.to(dev), want_zp=True)
    dd, zz = delta.expand(n_tok) if not per_token else delta, zp.expand(n_tok) if not per_token else zp
    _check_exact(qa, None, x, n_bits, None, "static B%d C%d" % (B, C), delta=dd, zp=zz)
    codes, dq = fq.static_act_quant(x.float(), dd.reshape(1, n_tok, 1), zz.reshape(1, n_tok, 1), n_bits)
    out, got, _, _ = ops.fakequant_act(x.to(dev), n_bits, delta=delta.to(dev), zp=zp.to(dev), want_codes=True)
    assert torch.equal(got.cpu().int(), codes.int()), _first_diff(got.cpu().int(), codes.int(), "fakequant static codes")
    assert torch.equal(out.cpu(), dq.half())


@pytest.mark.parametrize("n_bits", [8, 6])
@pytest.mark.parametrize("B,C", [(2, 96), (1, 1152)])
def test_fakequant_act_dynamic_edges(ops, dev, B, C, n_bits):
    """fq_stats / fq_finalize / fq_apply (the IEEE form, eps fill included) on Q1 and Q3: clean rows, and the whole Q3 sweep
    with its rows under 1e-6 (the oracle then refills every delta, and so does this kernel chain)."""
    q1 = qr.q1(B, 48, C, n_bits)
    q3 = qr.q3(B, C, qr.q3_magnitudes(49))
    good = qr.split_eps(q3, n_bits)[0]
    for x, want_eps in ((torch.cat([q1, q3[:, good]], 1), False), (q3, True)):
        codes, dq, delta, zp, eps = fq.dyn_act_quant(x.float(), n_bits)
        assert eps == want_eps
        st = ops.new_status(dev)
        out, got, d, z = ops.fakequant_act(x.to(dev), n_bits, status=st, want_codes=True)
        assert torch.equal(d.cpu(), delta.reshape(-1)) and torch.equal(z.cpu(), zp.reshape(-1))
        assert torch.equal(got.cpu().int(), codes.int()), _first_diff(got.cpu().int(), codes.int(), "fakequant codes")
        assert torch.equal(out.cpu(), dq.half())
        assert int(st.item()) == int(eps)


# ----------------------------------------------------------------------------- quantizers fused into temporal attention
# entry point, T, S, H, D -> kernel: attn_temporal_quant_kernel (H < 16), attn_temporal_quant2_kernel (H = 16),
# attn_temporal_long_kernel (T = 17 .. 64)
TEMPORAL = [("quant", 16, 8, 8, 64), ("quant", 5, 9, 2, 32), ("quant", 16, 8, 16, 72), ("long", 17, 6, 4, 16),
            ("long", 64, 4, 8, 64), ("long", 64, 5, 16, 72)]


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("kind,T,S,H,D", TEMPORAL)
def test_fused_temporal_quantizer_edges(ops, dev, kind, T, S, H, D, smooth):
    """One-hot temporal attention (one hot key for all heads of a query row, lead >= R1_GAP) whose V rows are Q1, Q3 and Q6
    rows of width H * D: the attention output IS the hot V row, so the fused quantizer's codes and grid must be the
    oracle's quantizer of that row - exact ties included.  ``smooth``: behind the Q2 vector (near ties through
    rq_div_rcp)."""
    import attn_regimes as ar
    Cc, scale = H * D, D ** -0.5
    s = qr.q2_smooth(Cc) if smooth else None
    q3 = qr.q3(1, Cc, qr.q3_magnitudes(97))
    pool = torch.cat([qr.q1(1, 48, Cc, 8, fixed=smooth), q3[:, qr.split_eps(q3, 8, s)[0]], qr.q6(1, Cc)], 1)
    vrows = qr.thin(pool, S * T)[0]                                             # [S * T, Cc]: V row j of sequence s
    q, k, hot = qr.one_hot_qk(S, T, H, D, scale, seed=100 * T + D)
    v = vrows.reshape(S, T, H, D)

    def to_rows(t):        # [S, T, H, D] -> rows (t, s)
        return t.reshape(S, T, Cc).permute(1, 0, 2).reshape(T * S, Cc)

    qkv = torch.cat([to_rows(q), to_rows(k), to_rows(v)], 1).to(dev)
    o = torch.full((T * S, Cc), float("nan"), dtype=torch.float16, device=dev)
    st = ops.new_status(dev)
    sd = None if s is None else s.to(dev)
    if kind == "quant":
        qa = ops.attn_temporal_rowquant(qkv, qkv[:, Cc:], qkv[:, 2 * Cc:], 1, T, S, H, D, 3 * Cc, status=st, o=o, s=sd)
    else:
        qa = ops.attn_temporal_long(qkv, qkv[:, Cc:], qkv[:, 2 * Cc:], 1, T, S, H, D, 3 * Cc, o=o, quant=True, status=st, s=sd)
    assert qa is not None
    torch.cuda.synchronize()
    gp = ar.gaps(q, k, hot[:, :, None].expand(S, T, H).contiguous(), scale, [T] * S)          # [S, T, H]
    sel = (gp >= ar.R1_GAP).all(-1).permute(1, 0).reshape(T * S)                                  # rows (t, s)
    assert float(sel.double().mean()) >= 0.9
    want = to_rows(torch.stack([v[i][hot[i]] for i in range(S)]))                               # the hot V row of every query
    idx = sel.nonzero()[:, 0]
    assert torch.equal(o.cpu()[idx], want[idx]), "%s: the output is not the hot V row" % kind
    x = want[idx][None]
    codes, _, delta, zp, eps = fq.dyn_act_quant(qr.smoothed(x, s), 8)
    assert not eps
    got = qa.xq.cpu()[idx, :Cc].int() + 128
    assert torch.equal(got, codes[0].int()), _first_diff(got, codes[0].int(), "fused codes")
    assert bool((qa.xq[:, Cc:] == 0).all())
    assert torch.equal(qa.sx.cpu()[idx], delta.reshape(-1))
    zx = zp.reshape(-1).int() - 128
    assert torch.equal(qa.zx.cpu()[idx], zx)
    assert torch.equal(qa.R.cpu()[idx], (codes[0].int() - 128).sum(-1) - Cc * zx)
    if bool(sel.all()):
        assert int(st.item()) == 0


# ----------------------------------------------------------------------------- weights
@pytest.mark.parametrize("n_bits", [8, 6, 4])
@pytest.mark.parametrize("N,K", [(48, 96), (24, 1152)])
def test_weight_minmax_and_pack_edges(ops, dev, N, K, n_bits):
    """weight_minmax_kernel + pack_weight_kernel (IEEE form) on Q1 rows at the weight's bit width: exact ties in the codes,
    tie codes through the nibble packing at 4 bits."""
    W = qr.q1(1, N, K, n_bits)[0]
    delta, zp = fq.weight_params(W.float(), n_bits)
    codes, _ = fq.weight_fakequant(W.float(), delta, zp, n_bits)
    for t in range(N):
        lo, _, k = qr.q1_row_spec(t, n_bits)
        assert float(delta[t]) == 2.0 ** -k and float(zp[t]) == -lo
    st = ops.new_status(dev)
    d, z = ops.weight_minmax(W.to(dev), n_bits, status=st)
    assert torch.equal(d.cpu(), delta.reshape(-1)) and torch.equal(z.cpu(), zp.reshape(-1))
    assert int(st.item()) == 0
    pw = ops.pack_weight(W.to(dev), d, z, n_bits)
    cw = 128 if n_bits == 8 else 0
    if n_bits <= 4:
        w32 = pw.wq.cpu().reshape(N, -1, 4).int()               # bytes of each uint32 group: low nibbles k0 + j, high k0 + 4 + j
        got = torch.cat([w32 & 0xF, (w32 >> 4) & 0xF], dim=-1).reshape(N, -1)
        assert bool((got[:, K:] == 0).all()) or pw.Kp == K
        got = got[:, :K]
    else:
        got = pw.wq.cpu().int()[:, :K] + cw
        assert bool((pw.wq[:, K:] == 0).all())
    assert torch.equal(got, codes.int()), _first_diff(got, codes.int(), "weight codes")
    assert torch.equal(pw.sw.cpu(), delta.reshape(-1))
    assert torch.equal(pw.zw.cpu(), zp.reshape(-1).int() - cw)
    assert torch.equal(pw.cs.cpu(), (codes.int() - cw).sum(-1))


# ----------------------------------------------------------------------------- GELU in front of the quantizer
def _gelu_input(B, C):
    q3 = qr.q3(B, C, qr.q3_magnitudes(49))
    return torch.cat([q3, qr.q5(B, C), qr.q6(B, C)], 1)


GELU_SPLIT = ((1, 8), (1, 6), (2, 8), (2, 6))


def _gelu_split_outputs(ops, dev):
    out = {}
    for B, bits in GELU_SPLIT:
        x = _gelu_input(B, 4608)
        for n in (x.shape[1], 3):                          # 3 rows: the partner waves of the odd tail write nothing
            q = ops.gelu_rowquant(qr.thin(x, n).to(dev), n_bits=bits)
            out[(B, bits, n)] = [t.cpu() for t in (q.xq, q.sx, q.zx, q.R)]
    return out


def test_gelu_rowquant_split_rows_edges(ops, dev, tmp_path):
    """C = 4608 without smoothing: rowquant_split_kernel (a row over two partner waves; B = 2: (sample, half)) against the
    one-row-per-wave kernels of a child process started with VQ_RQ_SPLIT=0, on Q3 / Q5 / Q6 rows (the extremum in either
    partner wave, in either sample): bit-identical, as in test_kernels_gpu.py."""
    code = ("import sys, torch; sys.path.insert(0, %r); sys.path.insert(0, %r); import viditq_amd; from viditq_amd import ops; "
            "import test_quantizer_edges_gpu as t\n"
            "with torch.no_grad():\n"
            "    torch.save(t._gelu_split_outputs(ops, torch.device('cuda:0')), sys.argv[1])\n" % (ROOT, os.path.join(ROOT, "tests")))
    f = str(tmp_path / "one_row.pt")
    r = subprocess.run([sys.executable, "-c", code, f], env=dict(os.environ, VQ_RQ_SPLIT="0"), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    ref = torch.load(f)
    got = _gelu_split_outputs(ops, dev)
    assert len(ref) == 2 * len(GELU_SPLIT)
    for key, want in ref.items():
        for name, g_, w_ in zip(FIELDS, got[key], want):
            assert torch.equal(g_, w_), (key, name)
        assert bool(torch.isfinite(got[key][1]).all())


@pytest.mark.parametrize("B,C", [(1, 4608), (1, 1152), (2, 4608), (2, 1152), (1, 320), (1, 1544), (2, 1544)])
def test_gelu_rowquant_fast_division_edges(ops, dev, B, C):
    """Smoothed GELU quantizers (C = 4608, 1544: rowquant_smooth_lds_kernel<GELU>, at 1544 with pad columns; else rowquant_fast_kernel<.., GELU>) with the
    reciprocal form against the same call with the IEEE division, on Q3 / Q5 / Q6: bit-identical, status included."""
    x = _gelu_input(B, C).to(dev)
    s = torch.exp(torch.randn(C, generator=torch.Generator().manual_seed(C + B)) * 0.7).float().to(dev)
    assert ops.smooth_rcp(s) is not None
    for bits in (8, 6):
        sa, sb = ops.new_status(dev), ops.new_status(dev)
        a = ops.gelu_rowquant(x, n_bits=bits, s=s, status=sa)
        b = ops.gelu_rowquant(x, n_bits=bits, s=s, status=sb, fast_div=False)
        for f in FIELDS:
            assert torch.equal(getattr(a, f), getattr(b, f)), (f, bits)
        assert int(sa.item()) == int(sb.item()) == 1            # the sweep holds rows under 1e-6
        assert bool(torch.isfinite(a.sx).all())
        assert bool((a.xq[:, C:] == 0).all())                    # pad columns [C, Kp)


# ----------------------------------------------------------------------------- LayerNorm + modulate in front of the quantizer
# B, C, outputs -> kernel: (1, 64, plain) ln_modulate_rowquant_fast_kernel<1>; (1, 1152, plain) ln_modulate_rowquant_half_kernel;
# (2, 1152, plain) its PAIR form; (1, 1152, one vector) smooth_rowquant_multi_kernel<LN, 1>; three vectors <LN, 3>;
# (1, 768, plain) / (2, 768, plain) the half-wave kernels at NIT = 6; (1, 64, two vectors) ln_modulate_rowquant_fast_kernel<1, 2>;
# (1, 1408, plain / three vectors) ln_modulate_rowquant_fast_kernel<3, 1> / <3, 3> (vectors without reciprocals in registers)
@pytest.mark.parametrize("name", qr.LN_FAMILIES)
@pytest.mark.parametrize("B,C,nout", [(1, 64, 0), (1, 1152, 0), (2, 1152, 0), (1, 1152, 1), (1, 1152, 3), (1, 768, 0), (2, 768, 0),
                                      (1, 64, 2), (1, 1408, 0), (1, 1408, 3)])
def test_ln_modulate_rowquant_edges(ops, dev, B, C, nout, name):
    """Q3 / Q5 / Q6 behind LayerNorm + modulate, against the oracle at the bounds of test_ln_modulate_rowquant (LN statistics
    differ from torch's in the last ulp: <= 1 code step on < 0.5 % of the elements, tight dequant parity, delta to 1e-5).
    test_quant_rows_cpu.py shows the oracle itself stays inside the 0.5 % on these rows when its statistics move by one ulp;
    no family had to be dropped."""
    x, shift, scale = qr.ln_inputs(name, B, C)
    n_tok = x.shape[1]
    smooth = [None] if nout == 0 else [(torch.rand(C, generator=torch.Generator().manual_seed(50 + j)) + 0.5).float()
                                       for j in range(nout)]
    xm = fq.t2i_modulate(fq.layernorm_noaffine(x.float()), shift[:, None, :], scale[:, None, :])
    st = ops.new_status(dev)
    outs = ops.ln_modulate_rowquant(x.to(dev), shift.to(dev), scale.to(dev), 1e-6,
                                    smooth=[None if s is None else s.to(dev) for s in smooth], status=st)
    for s, qa in zip(smooth, outs):
        xin = xm if s is None else xm / s
        codes, dq, delta, zp, eps = fq.dyn_act_quant(xin, 8)
        assert not eps
        got = qa.xq[:, :C].cpu().int().reshape(B, n_tok, C) + 128
        diff = (got - codes.int()).abs()
        print("%s B%d C%d nout%d: max code step %d, share %.3g" % (name, B, C, nout, int(diff.max()),
                                                                  float((diff > 0).float().mean())))
        assert int(diff.max()) <= 1
        assert float((diff > 0).float().mean()) < 5e-3
        got_dq = (got.float() - (qa.zx.cpu().reshape(B, n_tok, 1) + 128)) * qa.sx.cpu().reshape(B, n_tok, 1)
        rel = float((got_dq.double() - dq.double()).norm() / dq.double().norm())
        assert rel < 2e-3, rel
        for b in range(B):                                # the step of every sample's rows (the grid is shared over B)
            assert torch.allclose(qa.sx.cpu().reshape(B, n_tok)[b], delta.reshape(-1), rtol=1e-5)
        # the row term the int8 GEMM's zero-point correction reads, from the kernel's own codes (rq_write_row's identity)
        assert torch.equal(qa.R.cpu(), qa.xq.cpu().int().sum(-1).int() - C * qa.zx.cpu())
    assert int(st.item()) == 0
