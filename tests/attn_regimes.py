"""Attention inputs whose softmax scores have a known structure (peaked, stepped, shifted), for the kernel tests of
test_attention_softmax_gpu.py and the CPU checks of test_attention_regimes_cpu.py.

Every regime is stated in the exp2 domain s * scale * log2(e), where the kernels compare scores.  Tensors are fp16 on
the CPU, laid out [n, L, H, D] (n sequences; for temporal attention a sequence is the T frames of one (b, s)).  Key
lengths may differ per sequence (`lens`): rows past a sequence's length are zero and are not keys.  All scores stay
within ~300 in magnitude, so that fp32 summation order moves no softmax weight by more than ~1e-4.

R1  one-hot: query i = lam * k[j(i)], keys nearly orthogonal; the hot key leads the second best by >= 60.
R2  staircase / sawtooth on channel D-1: each `step`-key tile leads the previous one by `lead` (rising) or trails it
    (falling); the other channels are small noise.  Both the deferred (lead < 8) and the taken (lead > 8) rescale of
    the flash kernels run on late tiles.
R3  common shift on channel D-1: every score of row i moves by +shift (even i) or -shift (odd i) on top of N(0,1)
    base scores.  The softmax is invariant under it.
"""
import math

import torch

LOG2E = 1.4426950408889634
DSTAR = -1                      # the dedicated channel of R2 / R3: d* = D - 1
R1_SCORE = 280.0                # the hot key's score (exp2 domain)
R1_MAX_COS = 0.75               # largest cosine between two keys of a sequence: gap >= 280 * (1 - 0.75) = 70
R1_GAP = 60.0                   # rows at least this far ahead return the hot V row exactly
R2_MAX = 250.0


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def hot_sweep(Lk):
    """The hot key of query row i is sweep[(i + h) % len(sweep)]: key 0, key Lk-1, every key of the ragged last 64-key
    tile, and one key of every residue mod 64 (hence mod 32 and mod 16) spread over the tiles, first tile included."""
    nt = max(1, Lk // 64)
    sw = [0, Lk - 1] + list(range(64 * (Lk // 64), Lk)) + list(range(min(64, Lk)))
    sw += [r + 64 * ((5 * r + 1) % nt) for r in range(64) if r + 64 * ((5 * r + 1) % nt) < Lk]
    return sw


def _unit_keys(L, D, g):
    """L nearly orthogonal directions of length sqrt(D) (resampled until no two have cosine > R1_MAX_COS)."""
    k = torch.randn(L, D, generator=g, dtype=torch.float64)
    for _ in range(200):
        k = k / k.norm(dim=1, keepdim=True)
        c = k @ k.T
        c.fill_diagonal_(-1.0)
        bad = (c > R1_MAX_COS).any(1)
        bad &= torch.arange(L) > c.argmax(1)          # resample one key of each close pair
        if not bool(bad.any()):
            break
        k[bad] = torch.randn(int(bad.sum()), D, generator=g, dtype=torch.float64)
    return k * math.sqrt(D)


def r1(n, Lq, lens, H, D, scale, seed):
    """One-hot rows.  Returns q, k, v and hot [n, Lq, H] (index of the hot key)."""
    g = _gen(seed)
    Lk = max(lens)
    lam = R1_SCORE / (D * scale * LOG2E)
    q = torch.zeros(n, Lq, H, D, dtype=torch.float64)
    k = torch.zeros(n, Lk, H, D, dtype=torch.float64)
    hot = torch.zeros(n, Lq, H, dtype=torch.long)
    for s in range(n):
        L = lens[s]
        sw = torch.tensor(hot_sweep(L))
        for h in range(H):
            k[s, :L, h] = _unit_keys(L, D, g)
            j = sw[(torch.arange(Lq) + h + s) % len(sw)]
            hot[s, :, h] = j
            q[s, :, h] = lam * k[s, j, h]
    v = torch.randn(n, Lk, H, D, generator=g)
    for s in range(n):
        v[s, lens[s]:] = 0
    return q.half(), k.half(), v.half(), hot


def r2_profile(Lk, step, lead, falling):
    """g(j) of the staircase: +lead per `step`-key tile, a sawtooth of period P tiles so that max g <= R2_MAX."""
    P = int(R2_MAX // lead) + 1
    t = torch.arange(Lk) // step % P
    return lead * ((P - 1 - t) if falling else t).double()


def _noise_sd(D, scale):
    # N(0, 0.3^2) channels at scale D^-0.5; the same spread in the exp2 domain at any other scale
    return 0.3 * math.sqrt(D ** -0.5 / scale)


def r2(n, Lq, lens, H, D, scale, seed, step, lead, falling):
    g = _gen(seed)
    Lk = max(lens)
    sd = _noise_sd(D, scale)
    beta = math.sqrt(R2_MAX / (scale * LOG2E))
    q = torch.randn(n, Lq, H, D, generator=g, dtype=torch.float64) * sd
    k = torch.randn(n, Lk, H, D, generator=g, dtype=torch.float64) * sd
    q[..., DSTAR] = beta
    prof = r2_profile(Lk, step, lead, falling) / (beta * scale * LOG2E)
    k[..., DSTAR] = prof[None, :, None]
    v = torch.randn(n, Lk, H, D, generator=g)
    for s in range(n):
        k[s, lens[s]:] = 0
        v[s, lens[s]:] = 0
    return q.half(), k.half(), v.half()


def r3(n, Lq, lens, H, D, scale, seed, shift):
    g = _gen(seed)
    Lk = max(lens)
    a = math.sqrt(shift / (scale * LOG2E))
    q = torch.randn(n, Lq, H, D, generator=g, dtype=torch.float64)
    k = torch.randn(n, Lk, H, D, generator=g, dtype=torch.float64)
    sign = 1.0 - 2.0 * (torch.arange(Lq) % 2).double()
    q[..., DSTAR] = a * sign[None, :, None]
    k[..., DSTAR] = a
    v = torch.randn(n, Lk, H, D, generator=g)
    for s in range(n):
        k[s, lens[s]:] = 0
        v[s, lens[s]:] = 0
    return q.half(), k.half(), v.half()


def build(regime, n, Lq, lens, H, D, scale, seed):
    """regime: ("R1",) | ("R2", step, lead, falling) | ("R3", shift).  Returns q, k, v, hot (None unless R1)."""
    if regime[0] == "R1":
        return r1(n, Lq, lens, H, D, scale, seed)
    if regime[0] == "R2":
        return r2(n, Lq, lens, H, D, scale, seed, *regime[1:]) + (None,)
    return r3(n, Lq, lens, H, D, scale, seed, regime[1]) + (None,)


def scores(q, k, scale, lens, rows=None):
    """fp64 scores in the exp2 domain [n, H, r, Lk] of the fp16 tensors (query rows `rows`), -inf past each length."""
    qq = q.double() if rows is None else q[:, rows].double()
    s = torch.einsum("nqhd,nkhd->nhqk", qq, k.double()) * (scale * LOG2E)
    for i, L in enumerate(lens):
        s[i, :, :, L:] = -math.inf
    return s


def gaps(q, k, hot, scale, lens, rows=None):
    """[n, r, H]: score of the hot key minus the best other key (negative when another key wins)."""
    s = scores(q, k, scale, lens, rows)
    hh = (hot if rows is None else hot[:, rows]).permute(0, 2, 1)           # [n, H, r]
    top = s.gather(-1, hh[..., None])[..., 0]
    s = s.scatter(-1, hh[..., None], -math.inf)
    return (top - s.max(-1).values).permute(0, 2, 1)


def attn_ref(q, k, v, scale, lens, rows=None):
    """fp64 softmax attention of the fp16 tensors: [n, r, H, D]."""
    s = scores(q, k, scale, lens, rows) / LOG2E
    p = s.softmax(-1)
    return torch.einsum("nhqk,nkhd->nqhd", p, v.double())


def sample_rows(Lq, tile, want=128):
    """Every `Lq // want`-th query row plus the first and last row of every `tile`-row query tile."""
    rows = set(range(0, Lq, max(1, Lq // want)))
    for t0 in range(0, Lq, tile):
        rows.update((t0, min(Lq, t0 + tile) - 1))
    return torch.tensor(sorted(rows))


# ----------------------------------------------------------------------------- the kernel table
def kernel_ids():
    """VQ_ATTN_K_* of include/viditq.h: {name: id}."""
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "viditq.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (VQ_ATTN_K_\w+) (\d+)", hdr)}


# kernels of the product dispatch (every VQ_ATTN_K_* id of include/viditq.h) and the temporal entry points
FWD_KERNELS = ["VQ_ATTN_K_FWD", "VQ_ATTN_K_FWD8_NW4", "VQ_ATTN_K_FWD8_NW8", "VQ_ATTN_K_FWD32D", "VQ_ATTN_K_FWD64D",
               "VQ_ATTN_K_CROSS32_2", "VQ_ATTN_K_CROSS32_3", "VQ_ATTN_K_CROSS32_4", "VQ_ATTN_K_CROSS32_5",
               "VQ_ATTN_K_CROSS_REG"]
TEMPORAL_KERNELS = ["attn_temporal", "attn_temporal_quant", "attn_temporal_quant2", "attn_temporal_long"]

# (kernel, D, shape): fwd shapes are n, Lq, lens, H, kv_off (the Lk argument is max(lens) unless "bound" says otherwise);
# temporal shapes are B, T, S, H.  FWD8_NW8 keeps K / V rows 2^19 elements apart in one 2 GiB buffer.
_SHAPES = [
    ("VQ_ATTN_K_CROSS32_2", 16, dict(n=2, Lq=300, lens=[100, 100], H=2, kv_off=False)),
    ("VQ_ATTN_K_CROSS32_2", 32, dict(n=2, Lq=300, lens=[128, 128], H=2, kv_off=False)),
    ("VQ_ATTN_K_CROSS32_2", 64, dict(n=2, Lq=257, lens=[65, 33], H=2, kv_off=True)),
    ("VQ_ATTN_K_CROSS32_2", 72, dict(n=2, Lq=300, lens=[120, 37], H=2, kv_off=True)),
    ("VQ_ATTN_K_CROSS32_3", 64, dict(n=2, Lq=300, lens=[150, 129], H=2, kv_off=True)),
    ("VQ_ATTN_K_CROSS32_3", 72, dict(n=2, Lq=256, lens=[192, 17], H=2, kv_off=True)),
    ("VQ_ATTN_K_CROSS32_4", 64, dict(n=2, Lq=260, lens=[256, 200], H=2, kv_off=True)),
    ("VQ_ATTN_K_CROSS32_4", 72, dict(n=2, Lq=300, lens=[250, 193], H=2, kv_off=True)),
    ("VQ_ATTN_K_CROSS32_5", 64, dict(n=2, Lq=300, lens=[320, 257], H=2, kv_off=True)),
    ("VQ_ATTN_K_CROSS32_5", 72, dict(n=2, Lq=290, lens=[300, 1], H=2, kv_off=True)),
    ("VQ_ATTN_K_CROSS_REG", 72, dict(n=2, Lq=100, lens=[120, 120], H=8, kv_off=False)),
    ("VQ_ATTN_K_CROSS_REG", 72, dict(n=2, Lq=200, lens=[128, 77], H=8, kv_off=True)),
    ("VQ_ATTN_K_FWD32D", 16, dict(n=1, Lq=300, lens=[1000], H=2, kv_off=False)),
    ("VQ_ATTN_K_FWD32D", 32, dict(n=2, Lq=513, lens=[191, 191], H=2, kv_off=False)),
    ("VQ_ATTN_K_FWD32D", 64, dict(n=1, Lq=192, lens=[700], H=2, kv_off=False)),
    ("VQ_ATTN_K_FWD32D", 72, dict(n=2, Lq=300, lens=[333, 333], H=2, kv_off=False)),
    ("VQ_ATTN_K_FWD64D", 16, dict(n=1, Lq=2048, lens=[2100], H=1, kv_off=False)),
    ("VQ_ATTN_K_FWD64D", 32, dict(n=1, Lq=2049, lens=[2048], H=1, kv_off=False)),
    ("VQ_ATTN_K_FWD64D", 64, dict(n=1, Lq=2100, lens=[2077], H=1, kv_off=False)),
    ("VQ_ATTN_K_FWD64D", 72, dict(n=1, Lq=2048, lens=[4100], H=2, kv_off=False)),
    ("VQ_ATTN_K_FWD8_NW4", 16, dict(n=2, Lq=150, lens=[333, 333], H=2, kv_off=False)),
    ("VQ_ATTN_K_FWD8_NW4", 32, dict(n=1, Lq=96, lens=[1000], H=2, kv_off=False)),
    ("VQ_ATTN_K_FWD8_NW4", 64, dict(n=2, Lq=191, lens=[129, 129], H=2, kv_off=False)),
    ("VQ_ATTN_K_FWD8_NW4", 72, dict(n=1, Lq=160, lens=[700], H=3, kv_off=False)),
    ("VQ_ATTN_K_FWD8_NW8", 72, dict(n=1, Lq=256, lens=[2048], H=1, kv_off=False, kv_stride=1 << 19)),
    ("VQ_ATTN_K_FWD", 16, dict(n=2, Lq=300, lens=[150, 77], H=2, kv_off=True, bound=0)),
    ("VQ_ATTN_K_FWD", 32, dict(n=2, Lq=80, lens=[333, 333], H=2, kv_off=False)),
    ("VQ_ATTN_K_FWD", 64, dict(n=2, Lq=50, lens=[100, 100], H=2, kv_off=False)),
    ("VQ_ATTN_K_FWD", 72, dict(n=2, Lq=200, lens=[300, 129], H=2, kv_off=True, bound=0)),
    ("VQ_ATTN_K_FWD", 72, dict(n=2, Lq=64, lens=[200, 200], H=4, kv_off=False)),
    ("attn_temporal", 16, dict(B=2, T=13, S=5, H=4)),
    ("attn_temporal", 32, dict(B=1, T=16, S=8, H=2)),
    ("attn_temporal", 64, dict(B=1, T=16, S=6, H=8)),
    ("attn_temporal", 72, dict(B=1, T=16, S=9, H=16)),
    ("attn_temporal_quant", 16, dict(B=1, T=16, S=8, H=4)),
    ("attn_temporal_quant", 32, dict(B=1, T=5, S=9, H=2)),
    ("attn_temporal_quant", 64, dict(B=1, T=16, S=8, H=8)),
    ("attn_temporal_quant", 72, dict(B=1, T=16, S=7, H=4)),
    ("attn_temporal_quant2", 16, dict(B=1, T=16, S=8, H=16)),
    ("attn_temporal_quant2", 32, dict(B=1, T=16, S=5, H=16)),
    ("attn_temporal_quant2", 64, dict(B=1, T=9, S=8, H=16)),
    ("attn_temporal_quant2", 72, dict(B=1, T=16, S=8, H=16)),
    ("attn_temporal_long", 16, dict(B=1, T=17, S=6, H=4)),
    ("attn_temporal_long", 32, dict(B=1, T=33, S=5, H=2)),
    ("attn_temporal_long", 64, dict(B=1, T=64, S=4, H=8)),
    ("attn_temporal_long", 72, dict(B=1, T=64, S=5, H=16)),
    ("attn_temporal_long", 72, dict(B=1, T=12, S=6, H=4)),
]
LEADS = (7.0, 9.0, 24.0)


def cases():
    """Every (kernel, D, shape) under R1, R2 rising and falling, R3 at +-300 or +-150, and - every third shape - R1 and
    R2 at scale 1.0 and 0.02 (R4).  Each case: dict(id, kernel, D, shape, regime, scale)."""
    out = []
    for i, (kern, D, sh) in enumerate(_SHAPES):
        temporal = kern.startswith("attn_")
        L = sh["T"] if temporal else max(sh["lens"])
        steps = (4, 8, 16) if temporal and L <= 16 else (16, 32, 64) if temporal else (64, 32, 16)
        step = steps[i % 3] if temporal else (64, 64, 32, 16)[i % 4]
        lead_up, lead_down = LEADS[i % 3], LEADS[(i + 1) % 3]
        regs = [(("R1",), None), (("R2", step, lead_up, False), None), (("R2", step, lead_down, True), None),
                (("R3", 300.0 if i % 2 == 0 else 150.0), None)]
        if i % 3 == 0:
            regs += [(("R1",), 1.0), (("R2", step, 9.0, False), 0.02), (("R1",), 0.02), (("R2", step, 24.0, False), 1.0)]
        for reg, scale in regs:
            name = "%s-D%d-%s-%s%s" % (kern.replace("VQ_ATTN_K_", ""), D, "x".join(str(v) if not isinstance(v, list) else
                                                                              "+".join(map(str, v)) for v in sh.values()),
                                       reg[0], "" if reg[0] == "R1" else "-" + "-".join(str(x) for x in reg[1:]))
            if scale is not None:
                name += "-scale%g" % scale
            out.append(dict(id=name, kernel=kern, D=D, shape=sh, regime=reg,
                            scale=D ** -0.5 if scale is None else scale, seed=1000 + 17 * i + len(out) % 7))
    return out


def fwd_layout(case):
    """Launch arguments of a vq_attn_fwd case: K / V share rows (k | v column blocks), packed by offsets with kv_off,
    one dense block per sequence without, or rows `kv_stride` elements apart."""
    sh, D = case["shape"], case["D"]
    Cc = sh["H"] * D
    n, Lq, lens = sh["n"], sh["Lq"], sh["lens"]
    kv_tok = sh.get("kv_stride", 2 * Cc)
    if sh["kv_off"]:
        kv_seq, Lk = 0, sh.get("bound", max(lens))
        offs = [0]
        for L in lens:
            offs.append(offs[-1] + L)
        kv_rows = offs[-1]
    else:
        assert len(set(lens)) == 1
        kv_seq, Lk, offs, kv_rows = lens[0] * kv_tok, lens[0], None, n * lens[0]
    return dict(n_seq=n, Lq=Lq, Lk=Lk, H=sh["H"], D=D, q_seq=Lq * Cc, q_tok=Cc, kv_seq=kv_seq, kv_tok=kv_tok,
                o_seq=Lq * Cc, o_tok=Cc, offs=offs, kv_rows=kv_rows)


def temporal_route(case):
    """The temporal kernel the entry point of a temporal case runs (vq_attn_temporal: T <= 16; the fused quantizer:
    attn_temporal_quant2_kernel for H == 16 with Kp <= 2048, attn_temporal_quant_kernel otherwise; vq_attn_temporal_long:
    T <= 64)."""
    sh, D = case["shape"], case["D"]
    kp = (sh["H"] * D + 127) // 128 * 128
    if case["kernel"] == "attn_temporal":
        return "attn_temporal" if sh["T"] <= 16 else None
    if case["kernel"] in ("attn_temporal_quant", "attn_temporal_quant2"):
        if sh["T"] > 16 or sh["H"] > 16 or sh["B"] != 1:
            return None
        return "attn_temporal_quant2" if sh["H"] == 16 and kp <= 2048 else "attn_temporal_quant"
    return "attn_temporal_long" if sh["T"] <= 64 and sh["H"] <= 16 else None
