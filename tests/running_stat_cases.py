"""Inputs and expected states of the running smooth-quant statistic (vq_act_scale_momentum, include/viditq.h), built in
torch / numpy on the CPU from the INTEGER-MAX model of its contract:

    m[b][c]  = max over tok of (bits(x[b, tok, c]) & 0x7fff), read back as fp16
    cur[c]   = (float(m[0][c]) + float(m[1][c]) + ...) / B
    state    = cur                                            when every entry of the state is zero
             = RN(RN(state * mom) + RN(cur * (1 - mom)))      otherwise, (1 - mom) evaluated in double, rounded once to fp32
    state[state == 0] = 1e-5

tests/test_running_smooth_cpu.py proves every case equal, bit for bit, to QuantLayer._update_running_act_scale followed
by the zero patch of QuantLayer.channel_wise_scale on the CPU; tests/test_running_smooth_gpu.py holds the kernel to the same
expectations.  A case is three consecutive calls (first-call branch, then the momentum branch twice) from ``init``.
Cases are built on demand from their names (seeded): nothing is kept between tests.
"""
import zlib

import numpy as np
import torch

MOMENTUM = 0.95
N_CALLS = 3


# ------------------------------------------------------------------------------------------------ the model
def model_step(x, state, momentum=MOMENTUM):
    """(new state [C] fp32, cur [C] fp32) for x [B, n_tok, C] fp16 and state [C] fp32 (not modified)."""
    B, n_tok, C = x.shape
    bits = x.contiguous().view(torch.int16).to(torch.int32) & 0x7fff
    m = bits.amax(dim=1).to(torch.int16).view(torch.float16).float().numpy()          # [B, C]
    acc = np.zeros(C, dtype=np.float32)
    for b in range(B):
        acc = (acc + m[b]).astype(np.float32)
    cur = (acc / np.float32(B)).astype(np.float32)
    st = state.numpy().astype(np.float32)
    if not (st != 0).any():
        new = cur.copy()
    else:
        mf, om = np.float32(momentum), np.float32(1.0 - momentum)
        new = ((st * mf).astype(np.float32) + (cur * om).astype(np.float32)).astype(np.float32)
    new[new == 0] = np.float32(1.0e-5)
    return torch.from_numpy(new), torch.from_numpy(cur)


# ------------------------------------------------------------------------------------------------ the cases
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _rand(g, B, n, C, scale=3.0):
    return (torch.randn(B, n, C, generator=g) * scale).half()


RANDOM = ["random/B%d_n%d_C%d" % (B, n, C) for B in (1, 2, 3) for n in (1, 7, 300, 1025) for C in (8, 72, 1152, 4608)]
SPECIAL = ["zero_column/B2_n37_C72", "zero_column/B1_n300_C1152",
           "extremes/B2_n37_C72", "extremes/B3_n300_C520",
           "peak_first_row/B2_n300_C1152", "peak_last_row/B2_n300_C1152", "peak_last_row_of_sample0/B2_n300_C1152",
           "peak_last_row/B1_n1025_C72",
           "one_nonzero_entry/B2_n37_C72", "one_nonzero_entry/B1_n300_C1152"]
NAMES = RANDOM + SPECIAL


def _shape(name):
    f = name.split("/")[1].split("_")
    return int(f[0][1:]), int(f[1][1:]), int(f[2][1:])


def inputs(name):
    """(xs: N_CALLS tensors [B, n_tok, C] fp16, init: [C] fp32 initial state)."""
    fam = name.split("/")[0]
    B, n, C = _shape(name)
    g = _gen(name)
    xs = [_rand(g, B, n, C, 3.0 if j == 0 else 2.0) for j in range(N_CALLS)]
    init = torch.zeros(C)
    if fam == "zero_column":
        # columns that are zero in EVERY call: the patch fires in the first call (cur = 0 -> 1e-5) and what it wrote is
        # what the momentum branch then decays; column 5 is zero in the first call only
        for x in xs:
            x[:, :, 3] = 0
            x[:, :, C - 1] = 0
        xs[0][:, :, 5] = 0
    elif fam == "extremes":
        for j, x in enumerate(xs):
            x[:, :, 0] = 0
            x[0, n // 2, 0] = -65504.0                               # the largest finite magnitude, negative
            x[:, :, 1] = 0
            x[B - 1, n - 1, 1] = -0.0                                # only signed zeros: the maximum is zero
            x[:, :, 2] = 0
            sub = torch.tensor([0x0001, 0x03ff - 0x8000, 0x0200], dtype=torch.int16).view(torch.float16)   # fp16 denormals, one negative
            x[0, 0, 2], x[B - 1, n - 1, 2], x[0, n // 3, 2] = sub[0], sub[1], sub[2]
            x[:, :, 3] = 0
            x[0, 0, 3] = torch.tensor([0x0001 + j], dtype=torch.int16).view(torch.float16)[0]      # the smallest denormals alone
            x[:, :, 4] = 65504.0 if j == 1 else -65504.0             # every row of every sample at the extreme
            x[B - 1, n - 1, C - 1] = 65504.0
    elif fam.startswith("peak_"):
        for x in xs:
            x.clamp_(-8.0, 8.0)
            row = {"peak_first_row": (0, 0), "peak_last_row": (B - 1, n - 1), "peak_last_row_of_sample0": (0, n - 1)}[fam]
            x[row[0], row[1], :] = torch.where(torch.arange(C) % 2 == 0, torch.tensor(-1000.0), torch.tensor(999.5)).half()
    elif fam == "one_nonzero_entry":
        init[C // 2] = 0.25                                          # NOT all zero: the momentum branch must run at once
    else:
        assert fam == "random"
    return xs, init


def expected(name, xs=None, init=None):
    """[(state after call j, cur of call j)] for the N_CALLS chained calls."""
    if xs is None:
        xs, init = inputs(name)
    out, st = [], init.clone()
    for x in xs:
        st, cur = model_step(x, st)
        out.append((st, cur))
    return out
