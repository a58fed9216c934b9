"""int8 GEMM operands whose output is known per element: for the kernel tests of test_gemm_exact_gpu.py and the CPU checks
of test_gemm_cases_cpu.py.

Every builder is plain torch on the CPU, seeded, and returns a ``Case``: the operands exactly as csrc/gemm_i8.hip reads
them (centred codes ``code - 128`` at 8 bits and ``code`` at 6 bits and below, k zero-padded to Kp = pad128(K),
R = rowsum - K zx, cs = sum(code - cw), nibble layout of csrc/pack.hip for n_bits <= 4) plus the int64 terms and the fp64
value of  y = sx sw (acc - zw R - zx cs) + b.

G1  address: one-hot activation rows (k(m) = (a m + c) mod K, value v(m)), weights f(n, k) over the whole code range,
    zero points 0, scales 1: y[m, n] = v(m) w[n, k(m)] names (m, n, k).  A gather, so usable at the benchmark sizes.
G2  exact dequant: full-range random codes and zero points (both ends planted), power-of-two sx[m] / sw[n] that move
    with the index, bias a multiple of every sx[m] sw[n].  ``prove_exact`` shows in int64 that every term and every
    partial sum of y is an integer multiple of S = sx sw below 2^24 S: exact in fp32 in ANY order, with or without fma,
    and in the integer form (|R|, |cs| < 2^23, |acc - zw R - zx cs| <= 2^24).  The expectation is exact.half(), bitwise.
G3  saturation: codes and zero points at the range ends, K = 4608 and 16380: acc = +-K 128 128, acc = 0 by
    cancellation, the largest |R|, |cs|, |zw R|, |zx cs|.  Not exact; bound = one fp16 ulp + 4 2^-24 S (|acc| + |zw R| +
    |zx cs|) + 4 2^-24 |b| (the bound of test_gemm_fp_dequant_under_adversarial_cancellation).  With the power-of-two
    scales used here U, V, P, Q and sx sw are exact, so an fp32 evaluation rounds float(acc), U P, V Q (2^-24 of one
    term each) and three sums (2^-24 of at most the sum of the magnitudes each): 4 2^-24 (sum) at most, in any order.
G4  fp16 store: G2-style exact operands (activation rows = their zero point everywhere but one k) whose y lands on
    chosen values: ties between fp16 neighbours of both parities, 65504, 65512, the fp32 predecessor of 65520, 65520,
    2^-24 and 2^-25, 0 by cancellation from both signs; with residuals (-half(y), sums that tie, sums across 65520)
    and power-of-two gates for VQ_EPI_RESID / VQ_EPI_GATE_RESID: half(float(resid) + g float(half(y))).
G5  GELU sweep: exact y from -24 to 12 in steps of 2^-6, 2^-10 .. 2^-24 around 0, and |y| up to 6e4.
"""
import math
from dataclasses import dataclass, field
from typing import Optional

import torch

TWO24 = 2 ** 24
BENCH_SHAPES = [(16384, 1152, 1152), (16384, 4608, 1152), (16384, 1152, 4608), (8192, 1152, 1152)]
RAGGED_SHAPES = [(1, 4, 1), (5, 292, 72), (130, 580, 200), (257, 1156, 1100), (300, 292, 1100), (513, 580, 72),
                 (300, 4, 200), (1, 1156, 72)]
INTERIOR_SHAPES = [(256, 288, 128), (512, 576, 256), (1024, 1152, 1152)]   # variant 19; 128-row form by default at 256 rows


def pad128(k):
    return (k + 127) // 128 * 128


def centre(n_bits):
    return 128 if n_bits == 8 else 0


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def pack_nibbles(codes):
    """[N, Kp] codes 0..15 -> [N, Kp / 2] uint8: byte j of each group of 8 k = code[k0 + j] | code[k0 + 4 + j] << 4."""
    N, Kp = codes.shape
    g = codes.reshape(N, Kp // 8, 2, 4).to(torch.int16)
    return (g[:, :, 0] | (g[:, :, 1] << 4)).reshape(N, Kp // 2).to(torch.uint8)


def unpack_nibbles(wq):
    """The decode of test_kernels_gpu.py (test_gemm_full_size_against_the_library_integer_matmul)."""
    N = wq.shape[0]
    g = wq.view(N, wq.shape[1] // 4, 4).to(torch.int16)
    return torch.cat([g & 15, g >> 4], dim=2).reshape(N, wq.shape[1] * 2).to(torch.int8)


@dataclass
class Case:
    name: str
    M: int
    N: int
    K: int
    a_bits: int
    w_bits: int
    xq: torch.Tensor            # [M, Kp] int8
    sx: torch.Tensor            # [M] fp32
    zx: torch.Tensor            # [M] int32
    R: torch.Tensor             # [M] int32
    wq: torch.Tensor            # [N, Kp] int8 or [N, Kp / 2] uint8
    sw: torch.Tensor            # [N] fp32
    zw: torch.Tensor            # [N] int32
    cs: torch.Tensor            # [N] int32
    bias: Optional[torch.Tensor]    # [N] fp32
    acc: Optional[torch.Tensor]     # [M, N] int64 (None for the gathers of G1)
    exact: torch.Tensor         # [M, N] fp64 (G1: int16) - y before the fp16 store
    x_raw: Optional[torch.Tensor] = None    # raw codes and zero points the operands were made of
    w_raw: Optional[torch.Tensor] = None
    zx_raw: Optional[torch.Tensor] = None
    zw_raw: Optional[torch.Tensor] = None
    extra: dict = field(default_factory=dict)

    @property
    def Kp(self):
        return pad128(self.K)

    def terms(self):
        """(t_w, t_x) = (zw R, zx cs) int64 [M, N]."""
        return self.zw.long()[None, :] * self.R.long()[:, None], self.zx.long()[:, None] * self.cs.long()[None, :]

    def S(self):
        return self.sx.double()[:, None] * self.sw.double()[None, :]

    def expect_half(self):
        """exact.half() for the exact families: the fp64 value is an fp32 number, so one rounding."""
        e32 = self.exact.float()
        assert torch.equal(e32.double(), self.exact.double())
        return e32.half()


def pack_operands(x_raw, zx_raw, a_bits, w_raw, zw_raw, w_bits):
    """Raw codes [M, K] / [N, K] and raw zero points -> the kernel's fields."""
    M, K = x_raw.shape
    N = w_raw.shape[0]
    Kp, cx, cw = pad128(K), centre(a_bits), centre(w_bits)
    assert int(x_raw.min()) >= 0 and int(x_raw.max()) < 2 ** a_bits and int(w_raw.min()) >= 0 and int(w_raw.max()) < 2 ** w_bits
    xq = torch.zeros(M, Kp, dtype=torch.int8)
    xq[:, :K] = (x_raw.long() - cx).to(torch.int8)
    zx = (zx_raw.long() - cx).to(torch.int32)
    R = (xq.long().sum(1) - K * zx.long()).to(torch.int32)
    wc = torch.zeros(N, Kp, dtype=torch.int8)
    wc[:, :K] = (w_raw.long() - cw).to(torch.int8)
    zw = (zw_raw.long() - cw).to(torch.int32)
    cs = wc.long().sum(1).to(torch.int32)
    wq = pack_nibbles(wc) if w_bits <= 4 else wc
    return xq, zx, R, wq, zw, cs, wc


def assemble(name, x_raw, zx_raw, a_bits, w_raw, zw_raw, w_bits, sx, sw, bias, extra=None):
    """A dense case: acc by an fp64 matmul of the centred codes (integers below 2^53: exact)."""
    M, K = x_raw.shape
    N = w_raw.shape[0]
    xq, zx, R, wq, zw, cs, wc = pack_operands(x_raw, zx_raw, a_bits, w_raw, zw_raw, w_bits)
    acc = (xq.double() @ wc.double().t()).long()
    c = Case(name, M, N, K, a_bits, w_bits, xq, sx.float(), zx, R, wq, sw.float(), zw, cs,
             None if bias is None else bias.float(), acc, None, x_raw, w_raw, zx_raw, zw_raw, extra or {})
    t_w, t_x = c.terms()
    tt = acc - t_w - t_x
    c.exact = c.S() * tt.double() + (0.0 if bias is None else c.bias.double()[None, :])
    return c


def _pow2(e):
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double())


def is_pow2(t):
    m, _ = torch.frexp(t.double())
    return bool((m == 0.5).all())


def prove_exact(c: Case):
    """int64 proof that y of ``c`` is exact in fp32 however it is associated, and in the integer form.  Returns the
    largest sum of term magnitudes in units of S (<= 2^24)."""
    assert is_pow2(c.sx) and is_pow2(c.sw)
    S = c.S()
    t_w, t_x = c.terms()
    if c.bias is None:
        bi = torch.zeros_like(c.acc)
    else:
        q = c.bias.double()[None, :] / S          # exact: a power-of-two divisor
        assert torch.equal(q, q.round())          # the bias is a multiple of every sx[m] sw[n]
        bi = q.long()
    total = c.acc.abs() + t_w.abs() + t_x.abs() + bi.abs()
    assert int(total.max()) <= TWO24, (c.name, int(total.max()))
    # integer form: 24-bit multiplies, int32 sum, one conversion
    assert int(c.R.abs().max()) < 2 ** 23 and int(c.cs.abs().max()) < 2 ** 23
    assert int(c.zx.abs().max()) <= 128 and int(c.zw.abs().max()) <= 128
    # scales keep every value a normal fp32 number: S 2^24 finite, S itself normal with 23 bits to spare below
    assert float(S.max()) * TWO24 < 2.0 ** 127 and float(S.min()) > 2.0 ** -100
    return int(total.max())


# --------------------------------------------------------------------------------------------------------------- G1
def g1_stride(K):
    """An odd stride coprime to K near K / 3: k(m) visits every k in K consecutive rows, neighbours far apart."""
    a = max(1, K // 3) | 1
    while math.gcd(a, K) != 1:
        a += 2
    return a


def g1_k(M, K):
    m = torch.arange(M)
    return (g1_stride(K) * m + (K - 1)) % K       # row 0 meets K - 1


def g1_v(M):
    m = torch.arange(M)
    return ((m % 7) + 1) * (1 - 2 * ((m // 7) % 2))      # 1 .. 7, sign flips every 7 rows


def g1_weights(N, K, w_bits):
    L = 2 ** w_bits
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    return (13 * n + 7 * k + (n // 16) * (k // 16) + 5 * (k // 128)) % L


def g1(M, N, K, w_bits):
    """Address family.  exact is int16 [M, N] (|v w| <= 7 * 128: an fp16 integer)."""
    kk, v = g1_k(M, K), g1_v(M)
    cx, cw = 128, centre(w_bits)
    Kp = pad128(K)
    xq = torch.zeros(M, Kp, dtype=torch.int8)
    xq[torch.arange(M), kk] = v.to(torch.int8)
    w_raw = g1_weights(N, K, w_bits)
    wc = torch.zeros(N, Kp, dtype=torch.int8)
    wc[:, :K] = (w_raw - cw).to(torch.int8)
    wq = pack_nibbles(wc) if w_bits <= 4 else wc
    zx = torch.zeros(M, dtype=torch.int32)
    zw = torch.zeros(N, dtype=torch.int32)
    R = v.to(torch.int32)                                   # rowsum - K * 0
    cs = wc.long().sum(1).to(torch.int32)
    exact = (wc[:, :K].t()[kk].to(torch.int16) * v.to(torch.int16)[:, None])      # gather: [M, N]
    return Case("g1_%dx%dx%d_w%d" % (M, N, K, w_bits), M, N, K, 8, w_bits, xq, torch.ones(M), zx, R, wq, torch.ones(N),
                zw, cs, None, None, exact, None, w_raw, zx + cx, zw + cw, {"k": kk, "v": v})


# --------------------------------------------------------------------------------------------------------------- G2
def g2_zero_points(n, n_bits, g, span=None):
    """Random raw zero points over the whole range (or +-span around its middle), both ends planted."""
    L = 2 ** n_bits
    if span is None:
        z = torch.randint(0, L, (n,), generator=g)
        z[0] = 0
        z[-1] = L - 1
        if n > 2:
            z[n // 2] = L - 1
            z[n // 2 - 1] = 0
    else:
        z = torch.randint(L // 2 - span, L // 2 + span + 1, (n,), generator=g)
    return z


def g2(M, N, K, a_bits=8, w_bits=8, seed=0, zw_span=None, bias=True):
    g = _gen(1000 * seed + M + 3 * N + 7 * K + a_bits + w_bits)
    x_raw = torch.randint(0, 2 ** a_bits, (M, K), generator=g)
    w_raw = torch.randint(0, 2 ** w_bits, (N, K), generator=g)
    if K >= 2:                       # both ends of the code range in every row: min-max of the dequantised row gives the grid back
        x_raw[:, 0], x_raw[:, -1] = 0, 2 ** a_bits - 1
        w_raw[:, -1], w_raw[:, 0] = 0, 2 ** w_bits - 1
    zx_raw = g2_zero_points(M, a_bits, g)
    zw_raw = g2_zero_points(N, w_bits, g, zw_span)
    sx = _pow2(-(8 + (torch.arange(M) * 5) % 4))             # 2^-8 .. 2^-11, neighbours differ
    sw = _pow2(-(8 + (torch.arange(N) * 3) % 5))             # 2^-8 .. 2^-12
    b = None
    if bias:
        bi = torch.randint(-1024, 1025, (N,), generator=g).double()
        b = bi * sw * 2.0 ** -8                              # a multiple of sx_max sw[n], hence of every sx[m] sw[n]
    c = assemble("g2_%dx%dx%d_a%dw%d" % (M, N, K, a_bits, w_bits), x_raw, zx_raw, a_bits, w_raw, zw_raw, w_bits, sx, sw, b)
    prove_exact(c)
    return c


def g2_zw_span(K, a_bits, w_bits):
    """Zero points of the weights narrowed where |zw R| alone (128 * 2 K 128 at 8 x 8 bits) would pass 2^24."""
    if K > 400 and a_bits == 8 and w_bits == 8:
        return 40
    if K > 400 and a_bits == 8 and w_bits == 6:
        return 24
    return None


def dequantised(raw, zp_raw, delta):
    """fp16 tensor (code - zp) delta: what the product quantizers are given in the builder-vs-packer tests."""
    v = (raw.double() - zp_raw.double()[:, None]) * delta.double()[:, None]
    assert torch.equal(v.half().double(), v)
    return v.half()


# --------------------------------------------------------------------------------------------------------------- G3
def g3(M, N, K, w_bits, seed=0):
    """Saturation.  Row / channel patterns cycle with the index: all low, all high, alternating high / low, alternating
    low / high (activations: +127 / -127, the one pattern a code off the range end, so that acc = 0 against a constant
    weight row at even K); zero points alternate between the range ends with a different period."""
    La, Lw = 256, 2 ** w_bits
    k = torch.arange(K)[None, :]
    alt = k % 2

    def pattern(idx, L, alt_lo):
        p = (idx % 4)[:, None]
        lo, hi, al = torch.zeros(1, 1, dtype=torch.long), torch.full((1, 1), L - 1), torch.full((1, 1), alt_lo)
        return torch.where(p == 0, lo, torch.where(p == 1, hi, torch.where(p == 2, torch.where(alt == 0, hi, al),
                                                                            torch.where(alt == 0, al, hi))))
    m, n = torch.arange(M), torch.arange(N)
    x_raw = pattern(m, La, 1).expand(M, K).contiguous()      # alternating rows: +127 / -127 (code 1), so that they cancel
    w_raw = pattern(n // 3, Lw, 0).expand(N, K).contiguous()
    zx_raw = torch.where((m // 4) % 2 == 0, 0, La - 1)
    zw_raw = torch.where((n // 12) % 2 == 0, Lw - 1, 0)
    sx = _pow2(-(11 + m % 3))
    sw = _pow2(-(6 + n % 4))                                 # S <= 2^-17: |y| <= 255 * 255 * 16380 * 2^-17 + |b| < 1e4
    g = _gen(77 + seed)
    b = (torch.randn(N, generator=g) * 50).float()
    c = assemble("g3_%dx%dx%d_w%d" % (M, N, K, w_bits), x_raw, zx_raw, 8, w_raw, zw_raw, w_bits, sx, sw, b)
    assert is_pow2(c.sx) and is_pow2(c.sw) and float(c.exact.abs().max()) < 65504
    return c


def g3_bound(c: Case):
    """(reference fp32 [M, N] = exact.half(), per-element bound)."""
    t_w, t_x = c.terms()
    ref = c.exact.half().float()
    ulp = 2.0 ** -10 * ref.abs().clamp(min=2.0 ** -14)
    slack = 4 * 2.0 ** -24 * (c.S() * (c.acc.abs() + t_w.abs() + t_x.abs()).double() + c.bias.abs().double()[None, :])
    return ref, ulp.double() + slack


# ----------------------------------------------------------------------------------------------------------- G4 / G5
G4_V = (1, -1, 2, -3)


def _zigzag(K):
    """0, 1, -1, 2, -2, ... : the K offsets nearest 0."""
    k = torch.arange(K)
    return ((k + 1) // 2) * torch.where(k % 2 == 1, 1, -1)





def landing_case(name, M, N, K, w_bits, classes, zx_zero, seed=0, v_list=G4_V):
    """Activation row m = its zero point everywhere and zero point + v(m) at k = m mod K; column n of class
    (e, centre_t) = classes[n % len]: sw = 2^e, weight codes sweep outwards along k from a code c0[n] that moves with the
    channel (so cs is large), bias = sw (centre_t - (c0 - zp_w)), sx = 1.  Then  y[m, n] = sw[n] v(m) (w[n, k] - zp_w[n])
    + b[n]  - at v = 1: sw (centre_t + 0, 1, -1, 2, -2, ... along k, as far as the code range goes before it wraps) - while
    acc, zw R and zx cs are as large as the zero points make them."""
    g = _gen(4000 + seed + M + N + K + w_bits)
    Lw = 2 ** w_bits
    m, n = torch.arange(M), torch.arange(N)
    kk = m % K
    v = torch.tensor(v_list)[(m // 4) % len(v_list)]
    zx_raw = torch.full((M,), 128) if zx_zero else g2_zero_points(M, 8, g).clamp(3, 253)
    x_raw = zx_raw[:, None].expand(M, K).contiguous()
    x_raw[m, kk] += v
    zw_raw = g2_zero_points(N, w_bits, g)
    c0 = Lw // 2 + ((5 * n) % (3 * Lw // 4 + 1) - 3 * Lw // 8 if w_bits > 4 else 0 * n)     # 8 bits: codes 32 .. 224
    w_raw = (c0[:, None] + _zigzag(K)[None, :]) % Lw
    cls = n % len(classes)
    e = torch.tensor([c[0] for c in classes])[cls]
    ct = torch.tensor([c[1] for c in classes], dtype=torch.long)[cls]
    sw = _pow2(e)
    bi = ct - (c0 - zw_raw)
    sx = torch.ones(M, dtype=torch.float64)
    b = bi.double() * sw
    c = assemble(name, x_raw, zx_raw, 8, w_raw, zw_raw, w_bits, sx, sw, b, {"k": kk, "v": v, "cls": cls})
    prove_exact(c)
    return c


# (exponent of sw, centre of the window in units of sw)
G4_TIES = [(-10, 4608), (-7, -6001), (-20, 3000), (-25, 0), (-4, 0), (3, 8189), (3, -8189), (-13, 5000)]
G4_EDGES = G4_TIES + [(-8, 65520 * 256 - 1), (-8, -(65520 * 256 - 1))]
G4_NORMAL = [(-10, 4608), (-7, -6001), (-20, 3000 * 64), (-4, 300), (-13, 5000), (-5, 4099), (-2, 7001), (-9, -4500)]


def g4(M, N, K, w_bits, edges=False):
    """Plain epilogue.  edges: every activation zero point in the middle (zx = 0) so that the bias may take nearly all
    of the 2^24 budget - the column classes of the fp32 predecessor of 65520."""
    return landing_case("g4_%dx%dx%d_w%d%s" % (M, N, K, w_bits, "_edges" if edges else ""), M, N, K, w_bits,
                        G4_EDGES if edges else G4_TIES, edges)


def g4_gates(M, N, rows_per_gate):
    ns = (M + rows_per_gate - 1) // rows_per_gate
    s, n = torch.arange(ns)[:, None], torch.arange(N)[None, :]
    return _pow2((s + n) % 3 - 1).float()                      # 0.5, 1, 2


def g4_resid(M, N, K, w_bits, rows_per_gate=0):
    """Residual epilogues.  Returns (case, resid fp16 [M, N], gate fp32 or None, expected fp16).  |y| stays in the
    normal fp16 range (so a power-of-two gate commutes with the store rounding: half(g y) = g half(y), asserted) and the
    residual of element (m, n) is, by (m + n) mod 4:  -g half(y);  a value two binades above the lowest set bit of
    g half(y), which makes the sum a tie;  +-65504 with the sign of y;  a seeded normal."""
    c = landing_case("g4r_%dx%dx%d_w%d_g%d" % (M, N, K, w_bits, rows_per_gate), M, N, K, w_bits, G4_NORMAL, False, seed=5)
    yh = c.expect_half()
    gate = None
    z = yh.float()
    if rows_per_gate:
        gate = g4_gates(M, N, rows_per_gate)
        gf = gate[torch.arange(M) // rows_per_gate]
        z = gf * yh.float()
        assert torch.equal((gf.double() * c.exact).float().half().float(), z)     # folded = un-folded gate
        assert float(z.abs().max()) < 65504 and float(z.abs()[z != 0].min()) >= 2.0 ** -14
    g = _gen(9 + M + N)
    kind = (torch.arange(M)[:, None] + torch.arange(N)[None, :]) % 4
    zd = z.double()
    mant, ex = torch.frexp(zd)                                   # z = mant 2^ex, mant in [0.5, 1): 11 bits
    mi = (mant.abs() * 2048).long()                              # 1024 .. 2047
    tz = torch.zeros_like(mi)                                    # trailing zero bits of mi
    for sh in range(1, 12):
        tz += ((mi % (1 << sh)) == 0).long()
    q = ex - 11 + tz                                             # lowest set bit of z = 2^q
    mz = mi >> tz                                                # odd
    j = (torch.arange(M)[:, None] + 2 * torch.arange(N)[None, :]) % 2
    r_tie = torch.sign(zd) * (1024 + j).double() * _pow2(q + 1)
    ok_tie = (z != 0) & (q + 12 <= 15) & (q + 11 >= -14) & (mz + 2 * j < 2040)     # r finite, normal; same binade
    r_edge = torch.sign(zd) * 65504.0
    r_rand = (torch.randn(M, N, generator=g) * 4).double()
    resid = torch.where(kind == 0, -zd, torch.where((kind == 1) & ok_tie, r_tie, torch.where(kind == 2, r_edge, r_rand)))
    resid = resid.float().half()
    expected = (resid.float() + z).half()                        # fp32 sum, then the store rounding
    c.extra.update(kind=kind, ok_tie=ok_tie)
    return c, resid, gate, expected


def g5_classes(w_bits, K):
    """y = 2^-6 t for every integer t from -24 * 64 to 12 * 64 (one window of min(codes, K) - 2 values per class); steps
    of 2^-10 .. 2^-24 around 0; more of the region whose result is an fp16 subnormal (y from -5.6 to -4.2); |y| up to 6e4
    (|t - centre| <= 255 where the codes wrap: |y| <= 16 * 4055 = 64880)."""
    W = (min(2 ** w_bits, K) - 2) // 2 * 2
    return ([(-6, c) for c in range(-1536 + W // 2 - 1, 768 + W, W)] +
            [(-10, 0), (-14, 0), (-18, 0), (-24, 0), (-8, 300), (-8, -1200), (-7, -700), (-7, -620), (-7, -540),
             (4, 3800), (4, -3800), (0, 12000), (0, -12000)])


def g5(M, N, K, w_bits):
    """GELU sweep (v = 1 in every row: a column's window is met value by value once M >= min(codes, K))."""
    return landing_case("g5_%dx%dx%d_w%d" % (M, N, K, w_bits), M, N, K, w_bits, g5_classes(w_bits, K), False, seed=11,
                        v_list=(1,))


# relative error of gelu_tanh_f (gemm_common.h): y = x rcp(1 + exp2(w)), w = x fma(x^2, c1, c2).
#   w: x^2, the fma and the product round once each, c1 and c2 are rounded constants: |dw| <= 5 2^-24 |w|, and
#   d(2^w) / 2^w = ln 2 dw <= ln 2 * 5 2^-24 * 126 (beyond |w| ~ 126 the exponential is 0 or inf and drops out);
#   v_exp_f32 and v_rcp_f32: 1 ulp = 2^-23 each; 1 + e and the final product: 2^-24 each.
#   d y / y = (e / (1 + e)) d e / e + ... <= the sum.
G5_REL = math.log(2) * 5 * 2.0 ** -24 * 126 + 2 * 2.0 ** -23 + 2 * 2.0 ** -24


def gelu_ref(y):
    """tanh-GELU of exact y in fp64: 0.5 y (1 + tanh(u)), u = sqrt(2 / pi) (y + 0.044715 y^3), evaluated as
    y / (1 + exp(-2 u)) - the same function without the cancellation of 1 + tanh(u) in the negative tail."""
    y = y.double()
    u = math.sqrt(2.0 / math.pi) * (y + 0.044715 * y ** 3)
    return y / (1.0 + torch.exp(-2.0 * u))


def gelu_formula_fp32(y):
    """gelu_tanh_f of gemm_common.h step by step in fp32 torch (separate multiply and add for the fma)."""
    x = y.float()
    x2 = x * x
    w = x * (x2 * (-0.044715 * 2.302208198) + (-2.302208198))
    e = torch.exp2(w)
    return x * (1.0 / (1.0 + e))


def g5_bound(ref):
    """one fp16 ulp of the reference (floor 2^-24) + the formula's relative error."""
    a = ref.abs()
    ex = torch.floor(torch.log2(a.clamp(min=2.0 ** -14)))
    ulp = torch.pow(torch.tensor(2.0, dtype=torch.float64), ex - 10).clamp(min=2.0 ** -24)
    return ulp + G5_REL * a


# ------------------------------------------------------------------------------------------------- CPU reference
MUTANTS = ("row_m1", "col_n1", "kswap", "nibswap", "droplast", "zpsign", "rtz")


def rtz_half(v):
    """fp64 -> fp16 rounding toward zero (finite stays finite)."""
    h = v.float().half()
    over = h.double().abs() > v.abs()
    bits = h.view(torch.int16)
    return torch.where(over, bits - 1, bits).view(torch.float16)     # sign-magnitude: one step toward zero


def reference(c: Case, mutant=None, order=0, dtype=torch.float64):
    """y [M, N] recomputed FROM THE PACKED OPERANDS the way the kernel reads them.  ``order``: association of the three
    terms (0: the documented  S acc + (U P + (V Q + b));  1: ((S acc + U P) + V Q) + b;  2: (S acc + V Q) + (U P + b)).
    ``dtype`` fp32 evaluates every product and sum in fp32.  ``mutant``: one wrong kernel (MUTANTS)."""
    M, N, K, Kp = c.M, c.N, c.K, c.Kp
    xs = c.xq.clone()
    ws = unpack_nibbles(c.wq) if c.w_bits <= 4 else c.wq.clone()
    if mutant == "nibswap":
        assert c.w_bits <= 4
        ws = ws.reshape(N, Kp // 8, 2, 4).flip(2).reshape(N, Kp)
    if mutant == "kswap":
        xs = xs.reshape(M, Kp // 32, 2, 16).flip(2).reshape(M, Kp)
    if mutant == "droplast":
        xs[:, Kp - 128:] = 0
    acc = (xs.double() @ ws.double().t())
    sx, zx, R = c.sx.clone(), c.zx.clone(), c.R.clone()
    sw, zw, cs = c.sw.clone(), c.zw.clone(), c.cs.clone()
    b = torch.zeros(N) if c.bias is None else c.bias.clone()
    if mutant == "row_m1":                       # last row of every 16-row fragment (and of the matrix) reads its neighbour
        idx = torch.arange(M)
        src = torch.where((idx % 16 == 15) | (idx == M - 1), (idx - 1).clamp(min=0), idx)
        sx, zx, R = sx[src], zx[src], R[src]
    if mutant == "col_n1":
        idx = torch.arange(N)
        src = torch.where(idx % 4 == 3, (idx + 1).clamp(max=N - 1), idx)
        src[N - 1] = max(N - 2, 0)
        sw, zw, cs, b = sw[src], zw[src], cs[src], b[src]
    t = dtype
    S = sx.to(t)[:, None] * sw.to(t)[None, :]
    U, V = sx.to(t) * R.to(t), sx.to(t) * (-zx).to(t)
    P, Q = sw.to(t) * (zw if mutant == "zpsign" else -zw).to(t), sw.to(t) * cs.to(t)
    A = S * acc.to(t)
    UP, VQ, bb = U[:, None] * P[None, :], V[:, None] * Q[None, :], b.to(t)[None, :]
    if order == 0:
        y = A + (UP + (VQ + bb))
    elif order == 1:
        y = ((A + UP) + VQ) + bb
    else:
        y = (A + VQ) + (UP + bb)
    return y


def reference_half(c, mutant=None):
    y = reference(c, None if mutant == "rtz" else mutant)
    return rtz_half(y) if mutant == "rtz" else y.float().half()


def first_mismatch(bad, BM=256, BN=288):
    """Name the first wrong element of a boolean [M, N] map: (m, n), its tile and its position inside the wave tile
    (gemm_wide.h: 4 x 2 waves; a lane owns token row lane & 15 of a 16-row fragment and channels 4 (lane >> 4) .. + 3)."""
    idx = torch.nonzero(bad)
    m, n = int(idx[0, 0]), int(idx[0, 1])
    wtm, wtn = BM // 4, BN // 2
    rm, rn = m % BM, n % BN
    lane = ((rn % wtn) % 16 // 4) * 16 + (rm % wtm) % 16
    return ("%d wrong of %d; first (m=%d, n=%d): tile (%d, %d) of %dx%d, wave (%d, %d), fragment (i=%d, j=%d), lane %d, "
            "element %d" % (idx.shape[0], bad.numel(), m, n, m // BM, n // BN, BM, BN, rm // wtm, rn // wtn,
                            (rm % wtm) // 16, (rn % wtn) // 16, lane, rn % 4))
