"""LayerNorm + modulate + quantizer under the margin-exact rule: inputs, the fp64 reference, the set of fp32 evaluations a
correct kernel may be, and the checker - for test_ln_modulate_exact_gpu.py (the kernels) and test_ln_cases_cpu.py (the
proof that a correct kernel cannot fail, and that wrong ones do).  Plain torch on the CPU; imports no GPU code.

The rule.  u64 = LN(x) * (1 + scale) + shift in fp64 from the fp16 x (biased variance, eps inside the square root), the
quantizer grid of u64 / s as the oracle's token_params in fp64 (rows shared over the batch, min <= 0 <= max,
delta = (max - min) / qmax), t64 = u64 / s / delta64, z64 = -min / delta64.  A kernel evaluates the same expressions in
fp32 in some order; the MODEL SET (models()) holds the orders the sources use and their neighbours, and E_t, E_u, E_z,
E_delta are, per token, the largest distance of any member from the reference.  A kernel output is then held EXACTLY,
except where the fp64 value lies within 4 E (codes and zero point: at least 2^-10 of a step; the fp16 activation: 1.5 E,
scaled by the element's own size, see XM_FACTOR) of a rounding boundary; there it may take either neighbour and nothing else.  No share of elements is excused and no row is left out; the share
of elements with two admissible values is itself capped (a property of the reference alone, asserted with the rest).

Row families (x [B, n, C] fp16, shift / scale [B, C] fp16-valued fp32):
  L1  N(0, 2^2); at B = 2 the samples' shift / scale differ strongly (scale -0.5 against +0.5, shift +1 against -1)
  L2  offset rows, mean 64, sigma 1 (one-pass variance, a mean taken after rounding)
  L3  values on a 2^-10 grid with variance between 0.25 eps and 4 eps, eps = 1e-6: run at eps = 1e-6 and 1e-5, the value
      and the placement of eps decide the codes
  L4  one massive channel per row, 50 - 200 times the rest, at column 0, C - 1 and the first / last column of a lane's chunk
  Q3 / Q5 / Q6  quant_rows.ln_inputs' rows
"""
import math

import torch

import quant_rows as qr
from oracle import fakequant as fq

FAMILIES = ("L3", "L1", "L2", "L4", "Q3", "Q5", "Q6")       # mixed() deals rows in this order: one row = L3 (eps matters)
FLOOR = 2.0 ** -10            # least margin of a code / zero point, in steps
FACTOR = 4.0                  # margin = FACTOR * E: evaluation orders outside the model set
XM_FACTOR = 1.5               # the same for the fp16 activation: the cap below cannot hold at 4 (L4 rows 3.5 %, Q5 2.7 %) nor at
#                               2 (L4 2.04 %): values near zero have fp16 steps below any fp32 error.  At 1.5: 1.63 % at most
CAP = 0.02                    # largest share of elements of one output with two admissible values (launches of fewer
CAP_COUNT = 3                 # than 150 elements - one row of 64 or 96 channels: at most 3 elements instead)
XM_ILL = ("L2", "L3")         # rows whose fp16 activation no fp32 evaluation determines: the mean alone rounds at ulp(64) =
XM_ILL_CAP = 0.5              # 7.6e-6 (L2) against fp16 steps of 5e-4, so a third of the elements have two values at any
#                               factor >= 1; they are still held to their two neighbours, under this cap of their own
E_T_SMALL = 1.0e-2            # "small": E_t and E_z (steps) of every family stay below (largest: L3 at 8 bits, 4.5e-3)
BLOCK_WIDTHS = (768, 1024, 1152, 1280)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _h(t):
    return t.half().float()


# ----------------------------------------------------------------------------- inputs
def l4_columns(C):
    """Column of the massive channel, by row: the row ends and both sides of a lane's chunk in either lane map (4 channels
    per lane at stride 128, 8 at stride 512)."""
    return [0, C - 1, 7 % C, 8 % C, 3, 4, 127 % C, 128 % C, 511 % C, 512 % C]


def family(name, B, n, C, seed=0):
    """n rows of one family: x [B, n, C] fp16, shift, scale [B, C] fp32 (fp16 values)."""
    g = _gen(9000 + seed + 17 * C + B)
    shift = _h(torch.randn(B, C, generator=g) * 0.3)
    scale = _h(torch.randn(B, C, generator=g) * 0.3)
    if name == "L1":
        x = (torch.randn(B, n, C, generator=g) * 2.0).half()
        if B == 2:
            scale = _h(torch.tensor([-0.5, 0.5]).reshape(2, 1) + torch.randn(B, C, generator=g) * 0.1)
            shift = _h(torch.tensor([1.0, -1.0]).reshape(2, 1) + torch.randn(B, C, generator=g) * 0.1)
    elif name == "L2":
        x = (64.0 + torch.randn(B, n, C, generator=g)).half()
    elif name == "L3":
        # k * 2^-10 around a base that moves with the row; sd of k cycles so that var / eps covers [0.25, 4]
        sd = torch.tensor([0.62, 1.0, 1.45, 1.9])[torch.arange(n) % 4].reshape(1, n, 1)
        base = torch.tensor([0.0, 0.25, -0.125])[torch.arange(n) % 3].reshape(1, n, 1)
        k = torch.round(torch.randn(B, n, C, generator=g) * sd)
        xd = base.double() + k.double() * 2.0 ** -10
        x = xd.half()
        assert torch.equal(x.double(), xd)
        var = xd.var(-1, unbiased=False)
        assert float(var.min()) >= 0.25e-6 and float(var.max()) <= 4.0e-6, (float(var.min()), float(var.max()))
    elif name == "L4":
        x = (torch.randn(B, n, C, generator=g) * 2.0).half()
        cols = l4_columns(C)
        for t in range(n):
            for b in range(B):
                i = t + 3 * b
                mag = 2.0 * (50.0 + 150.0 * ((7 * i) % 10) / 9.0)
                x[b, t, cols[i % len(cols)]] = mag if i % 2 == 0 else -mag
    else:
        x, shift, scale = qr.ln_inputs(name, B, C, seed)
        idx = torch.linspace(0, x.shape[1] - 1, n).long() if n <= x.shape[1] else torch.arange(n) % x.shape[1]
        x = x[:, idx].contiguous()
    return x.contiguous(), shift, scale


def mixed(B, n, C, seed=0):
    """One launch of n rows dealt from every family in turn (row t: family t % 7, its row t // 7).  The modulation vectors
    are L1's (a launch has one pair); every family is a statement about x rows, L1's strong contrast about shift / scale.
    -> x, shift, scale, names [n]."""
    per = -(-n // len(FAMILIES))
    rows = {f: family(f, B, per, C, seed)[0] for f in FAMILIES}
    _, shift, scale = family("L1", B, 1, C, seed)
    x = torch.stack([rows[FAMILIES[t % 7]][:, t // 7] for t in range(n)], 1)
    return x.contiguous(), shift, scale, [FAMILIES[t % 7] for t in range(n)]


def smooth_vectors(C, n, seed=0):
    """n smoothing vectors, log-normal over about a decade."""
    g = _gen(50 + seed + C)
    return [torch.exp(torch.randn(C, generator=g) * 0.5).float() for _ in range(n)]


# ----------------------------------------------------------------------------- fp64 reference
def modulated64(x, shift, scale, eps):
    xd = x.double()
    mu = xd.mean(-1, keepdim=True)
    var = ((xd - mu) ** 2).mean(-1, keepdim=True)
    y = (xd - mu) / torch.sqrt(var + eps)
    return y * (1.0 + scale.double()[:, None, :]) + shift.double()[:, None, :]


def _grid(v, n_bits):
    """token_params without the rounding of the zero point, in v's precision: delta [n], z = -min / delta [n]."""
    B, n, C = v.shape
    r = v.permute(1, 0, 2).reshape(n, B * C)
    lo = r.min(-1).values.clamp(max=0.0)
    hi = r.max(-1).values.clamp(min=0.0)
    delta = (hi - lo) / (2 ** n_bits - 1)
    return delta, -lo / delta


# ----------------------------------------------------------------------------- the model set (fp32)
def _tree(p):
    """Pairwise sum over the last dimension (a power of two): the lanes' butterfly."""
    while p.shape[-1] > 1:
        p = p[..., 0::2] + p[..., 1::2]
    return p[..., 0]


def _lane_sum(v, lanes, w, step, square=False, fma=False):
    """fp32 sum of the rows of v [.., C] (``square``: of their squares, each rounded, or - ``fma`` - accumulated unrounded)
    in a lane map's order: lane l adds its chunks (w channels at l * w + i * step) one value after the other, then the
    lanes are summed pairwise.  Columns beyond C add +0."""
    C = v.shape[-1]
    nch = -(-C // step)
    pad = torch.zeros(v.shape[:-1] + (nch * step - C,), dtype=v.dtype)
    q = torch.cat([v, pad], -1).reshape(v.shape[:-1] + (nch, lanes, w))
    acc = torch.zeros(v.shape[:-1] + (lanes,), dtype=torch.float32)
    for i in range(nch):
        for e in range(w):
            a = q[..., i, :, e]
            if not square:
                acc = acc + a
            elif fma:
                acc = (a.double() * a.double() + acc.double()).float()
            else:
                acc = acc + a * a
    return _tree(acc)


ORDERS = {"half": (32, 4, 128), "wave": (64, 8, 512)}


def stats32(x, eps, order, sq_fma=False):
    """(mean, rstd) [B, n, 1] fp32 as rq_ln_stats writes them, the row summed in ``order`` ('torch': torch's own mean);
    ``sq_fma``: the squares accumulated as fma(d, d, sq)."""
    xf = x.float()
    C = xf.shape[-1]
    inv = torch.tensor(1.0 / C, dtype=torch.float32)
    e32 = torch.tensor(eps, dtype=torch.float32)
    if order == "torch":
        mu = xf.mean(-1, keepdim=True)
        var = ((xf - mu) ** 2).mean(-1, keepdim=True)
    else:
        mu = (_lane_sum(xf, *ORDERS[order]) * inv)[..., None]
        d = xf - mu
        var = (_lane_sum(d, *ORDERS[order], square=True, fma=sq_fma) * inv)[..., None]
    return mu, 1.0 / torch.sqrt(var + e32)


def modulate32(x, mu, rstd, shift, scale, fma):
    y = (x.float() - mu) * rstd
    sc1 = 1.0 + scale[:, None, :]
    sh = shift[:, None, :]
    if fma:                                       # one rounding: the product is exact in fp64
        return (y.double() * sc1.double() + sh.double()).float()
    return y * sc1 + sh


def orders_of(C):
    return ("torch", "wave") + (("half",) if C in BLOCK_WIDTHS else ())


def models(x, shift, scale, eps):
    """[(name, u fp32 [B, n, C])]: the torch oracle; then, for the row summed in torch's, the wave map's and (at a block
    width) the half-wave map's order, mean and rstd each as computed and one ulp to either side, the modulate rounded
    once and twice; and both orders again with the squares accumulated by fma."""
    out = [("oracle", fq.t2i_modulate(fq.layernorm_noaffine(x.float(), eps), shift[:, None, :], scale[:, None, :]))]
    for order in orders_of(x.shape[-1]):
        mu0, r0 = stats32(x, eps, order)
        for dm in (None, True, False):
            mu = mu0 if dm is None else qr.ulp_step(mu0, dm)
            for dr in (None, True, False):
                r = r0 if dr is None else qr.ulp_step(r0, dr)
                for fma in (False, True):
                    name = "%s m%s r%s %s" % (order, {None: "0", True: "+", False: "-"}[dm],
                                              {None: "0", True: "+", False: "-"}[dr], "fma" if fma else "mul+add")
                    out.append((name, modulate32(x, mu, r, shift, scale, fma)))
        if order != "torch":
            mu, r = stats32(x, eps, order, sq_fma=True)
            for fma in (False, True):
                out.append(("%s sq-fma %s" % (order, "fma" if fma else "mul+add"), modulate32(x, mu, r, shift, scale, fma)))
    return out


def launch_of(u, s, n_bits, C, Kp=None, want_xm=True):
    """What a kernel that evaluates the modulated activation as u (fp32) writes: the oracle's dynamic quantizer of u / s."""
    B, n, _ = u.shape
    Kp = (C + 127) // 128 * 128 if Kp is None else Kp
    v = u if s is None else u / s
    codes, _, delta, zp, eps_fill = fq.dyn_act_quant(v, n_bits)
    cx = 128 if n_bits == 8 else 0
    xq = torch.zeros(B * n, Kp, dtype=torch.int8)
    xq[:, :C] = (codes.int() - cx).reshape(B * n, C).to(torch.int8)
    zx = (zp.reshape(1, n).expand(B, n).reshape(-1).int() - cx).contiguous()
    R = xq.int().sum(-1) - C * zx
    return {"xq": xq, "sx": delta.reshape(1, n).expand(B, n).reshape(-1).contiguous(), "zx": zx, "R": R.int(),
            "status": int(eps_fill), "xm": u.half() if want_xm else None}


# ----------------------------------------------------------------------------- reference + margins of one launch
def _ulp32(v):
    """One fp32 ulp at |v| (fp64 tensor)."""
    f = v.abs().float()
    return (torch.nextafter(f, torch.full_like(f, math.inf)) - f).double()


class Reference:
    """The fp64 reference of one launch and, per output (smoothing vector or None), the margins of the model set."""

    def __init__(self, x, shift, scale, eps, n_bits, smooth=(None,), names=None):
        """``names``: the family of every row (mixed()), for the cap of the fp16 activation."""
        self.B, self.n, self.C = x.shape
        self.names = list(names) if names is not None else [""] * self.n
        self.smooth = list(smooth)
        self.u64 = modulated64(x, shift, scale, eps)
        ms = models(x, shift, scale, eps)
        self.model_names = [m[0] for m in ms]
        self.model_u = [m[1] for m in ms]
        # fp16 margin: per token the largest model error, absolute and relative to the element's own size
        # w = |1 + scale| (1 + |y|) + |shift| (the error of u is a mean error times rstd (1 + scale), an rstd error times
        # y (1 + scale), and roundings relative to the terms); each bounds every member at every element, the smaller holds
        B, n, C = x.shape
        tok = lambda e: e.permute(1, 0, 2).reshape(n, B * C).max(-1).values.reshape(1, n, 1)      # noqa: E731
        sc1 = (1.0 + scale.double())[:, None, :]
        y64 = (self.u64 - shift.double()[:, None, :]) / sc1
        w = sc1.abs() * (1.0 + y64.abs()) + shift.double()[:, None, :].abs()
        err = torch.stack([(u.double() - self.u64).abs() for u in self.model_u]).max(0).values
        self.E_u = tok(err)
        self.E_u_rel = tok(err / w)
        self.m_u = XM_FACTOR * torch.minimum(self.E_u.expand_as(w), self.E_u_rel * w)
        self._grids(n_bits)

    def rebits(self, n_bits, smooth=None):
        """The same launch at another code width (and other smoothing vectors): the modulated part is shared."""
        import copy
        r = copy.copy(self)
        if smooth is not None:
            r.smooth = list(smooth)
        r._grids(n_bits)
        return r

    def _grids(self, n_bits):
        n = self.n
        B, C = self.B, self.C
        tok = lambda e: e.permute(1, 0, 2).reshape(n, B * C).max(-1).values.reshape(1, n, 1)      # noqa: E731
        self.n_bits, self.qmax, self.cx = n_bits, 2 ** n_bits - 1, 128 if n_bits == 8 else 0
        self.out = []
        for s in self.smooth:
            sd = 1.0 if s is None else s.double()
            v64 = self.u64 / sd
            d64, z64 = _grid(v64, n_bits)
            t64 = v64 / d64.reshape(1, n, 1)
            E_t, E_z, E_d = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
            for u in self.model_u:
                v = u if s is None else u / s
                d, z = _grid(v, n_bits)
                t = v / d.reshape(1, n, 1)
                E_t = torch.maximum(E_t, tok((t.double() - t64).abs()).reshape(n))
                E_z = torch.maximum(E_z, (z.double() - z64).abs())
                E_d = torch.maximum(E_d, (d.double() - d64).abs())
            self.out.append({"s": s, "t64": t64, "z64": z64, "d64": d64, "E_t": E_t, "E_z": E_z, "E_d": E_d,
                             "m_t": torch.clamp(FACTOR * E_t, min=FLOOR), "m_z": torch.clamp(FACTOR * E_z, min=FLOOR),
                             "d_bound": torch.maximum(FACTOR * E_d, 2.0 * _ulp32(d64))})

    # ---- what the tables print
    def code_share(self, j):
        o = self.out[j]
        t = o["t64"]
        return float((((t - torch.floor(t)) - 0.5).abs() < o["m_t"].reshape(1, -1, 1)).double().mean())

    def xm_share(self, ill=False):
        """Share of fp16 elements with two admissible values, over the rows outside (``ill``: inside) XM_ILL."""
        rows = torch.tensor([(nm in XM_ILL) == ill for nm in self.names])
        if not bool(rows.any()):
            return 0.0
        two = (self.u64 - self.m_u).half() != (self.u64 + self.m_u).half()
        return float(two[:, rows].double().mean())

    def figures(self):
        f = {"E_u": float(self.E_u.max()), "xm_share": self.xm_share(), "xm_share_ill": self.xm_share(True)}
        for j, o in enumerate(self.out):
            f["out%d" % j] = {"E_t": float(o["E_t"].max()), "E_z": float(o["E_z"].max()),
                              "E_delta_rel": float((o["E_d"] / o["d64"]).max()), "code_share": self.code_share(j)}
        return f

    def finite_and_small(self):
        ok = math.isfinite(float(self.E_u.max()))
        for o in self.out:
            ok = ok and math.isfinite(float(o["E_t"].max())) and float(o["E_t"].max()) < E_T_SMALL
            ok = ok and math.isfinite(float(o["E_z"].max())) and float(o["E_z"].max()) < E_T_SMALL
            ok = ok and bool((o["E_d"] < 1.0e-4 * o["d64"]).all()) and bool((o["d64"] >= 10 * qr.EPS).all())
        return ok


def _cap(numel, cap=CAP):
    return max(cap, (CAP_COUNT + 0.5) / numel)


def _where(bad):
    i = bad.nonzero()[0].tolist()
    return "%d bad, first at %s" % (int(bad.sum()), i)


def check_xm(ref, xm, what):
    """Every element of the fp16 activation lies in [fp16(u64 - m_u), fp16(u64 + m_u)] - one value, or two neighbours where
    u64 is within m_u of a rounding boundary (a few more on XM_ILL rows whose margin exceeds an fp16 step); at most CAP of
    the elements have more than one value (XM_ILL_CAP on the rows of XM_ILL)."""
    lo, hi = (ref.u64 - ref.m_u).half(), (ref.u64 + ref.m_u).half()
    share, ill = ref.xm_share(), ref.xm_share(True)
    assert share <= _cap(ref.u64.numel()), "%s: %.3g of the xm elements have two admissible values (cap %.3g)" % (what, share, CAP)
    assert ill <= XM_ILL_CAP, "%s: %.3g of the xm elements of %s rows have two admissible values" % (what, ill, XM_ILL)
    got = xm.reshape(ref.B, ref.n, ref.C)
    bad = ~((got >= lo) & (got <= hi))
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError("%s xm: %s: kernel %r, admissible %r / %r (u64 %.9g, margin %.3g)" % (
            what, _where(bad), float(got[i]), float(lo[i]), float(hi[i]), float(ref.u64[i]), float(ref.m_u[i])))
    return share


def _check_rows(ref, got, what):
    """R identity, zero pads - from the kernel's own outputs."""
    C = ref.C
    xq = got["xq"]
    assert xq.shape[0] == ref.B * ref.n and xq.shape[1] >= C
    assert bool((xq[:, C:] == 0).all()), what + ": pad columns are not zero"
    R = xq.int().sum(-1) - C * got["zx"].int()
    bad = got["R"].int() != R
    assert not bool(bad.any()), "%s R: %s: kernel %d, sum(xq) - C zx = %d" % (
        what, _where(bad), int(got["R"][bad][0]), int(R[bad][0]))


def check_launch(ref, j, got, what):
    """The whole assertion set for output j of one dynamic launch.  ``got``: xq [B n, Kp] int8, sx, zx, R [B n], status,
    xm [B, n, C] fp16 or None - CPU tensors.  Returns the shares of elements with two admissible values."""
    o = ref.out[j]
    B, n, C, qmax, cx = ref.B, ref.n, ref.C, ref.qmax, ref.cx
    assert got["status"] == 0, "%s: status %d" % (what, got["status"])
    _check_rows(ref, got, what)
    # step: every row of every sample
    sx = got["sx"].double().reshape(B, n)
    bad = ~((sx - o["d64"].reshape(1, n)).abs() <= o["d_bound"].reshape(1, n))
    assert not bool(bad.any()), "%s sx: %s: kernel %.9g, reference %.9g" % (
        what, _where(bad), float(sx[bad][0]), float(o["d64"].reshape(1, n).expand(B, n)[bad][0]))
    # zero point
    zp = got["zx"].long().reshape(B, n) + cx
    z_lo = torch.round(o["z64"] - o["m_z"]).long().reshape(1, n)
    z_hi = torch.round(o["z64"] + o["m_z"]).long().reshape(1, n)
    bad = (zp != z_lo) & (zp != z_hi)
    assert not bool(bad.any()), "%s zx: %s: kernel zero point %d, z64 %.6f" % (
        what, _where(bad), int(zp[bad][0]), float(o["z64"].reshape(1, n).expand(B, n)[bad][0]))
    # codes, on the kernel's own zero point: exact outside the margin, the tie's two sides inside, clamped to [0, qmax]
    t, m = o["t64"], o["m_t"].reshape(1, n, 1)
    share = float((((t - torch.floor(t)) - 0.5).abs() < m).double().mean())
    assert share <= _cap(t.numel()), "%s: %.3g of the codes lie inside the tie margin (cap %.3g)" % (what, share, CAP)
    c_lo = (torch.round(t - m).long() + zp[:, :, None]).clamp(0, qmax)
    c_hi = (torch.round(t + m).long() + zp[:, :, None]).clamp(0, qmax)
    code = got["xq"][:, :C].long().reshape(B, n, C) + cx
    bad = (code != c_lo) & (code != c_hi)
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError("%s codes: %s: kernel %d, admissible %d / %d (t64 %.6f, zero point %d, margin %.3g)" % (
            what, _where(bad), int(code[i]), int(c_lo[i]), int(c_hi[i]), float(t[i]), int(zp[i[0], i[1]]), float(m[0, i[1], 0])))
    shares = {"codes": share}
    if got.get("xm") is not None:
        shares["xm"] = check_xm(ref, got["xm"], what)
    return shares


# ----------------------------------------------------------------------------- the static arm
def static_grids(ref, per_token, n_out):
    """Calibrated grids for a launch, from the reference alone: the range of the modulated activation (per token or of the
    whole tensor) over qmax, times 0.8 (centred: a tenth of the range clamps at either end), 1.0 and 1.3.
    -> delta, zp (integer-valued): n_out x [n or 1] fp32."""
    r = ref.u64.permute(1, 0, 2).reshape(ref.n, -1)
    lo, hi = r.min(-1).values.clamp(max=0.0), r.max(-1).values.clamp(min=0.0)
    if not per_token:
        lo, hi = lo.min().reshape(1), hi.max().reshape(1)
    ds = [(f * (hi - lo) / ref.qmax).float() for f in (0.8, 1.0, 1.3)][:n_out]
    los = [(lo + 0.1 * (hi - lo)).float(), lo.float(), lo.float()]
    return ds, [torch.round(-l / d) for l, d in zip(los, ds)]


def check_static(ref, j, got, delta, zp, what):
    """Output j of a static-grid launch behind LayerNorm + modulate: the grid is the caller's (sx, zx exact), the codes are
    the oracle's static quantizer of an admissible fp16 activation (of the kernel's own xm, bit for bit, when it is
    returned), R identity, pads.  ``xm`` [B, n, C] or None."""
    B, n, C, cx = ref.B, ref.n, ref.C, ref.cx
    s = ref.smooth[j]
    d = delta.reshape(-1).expand(n) if delta.numel() == 1 else delta.reshape(-1)
    z = zp.reshape(-1).expand(n) if zp.numel() == 1 else zp.reshape(-1)
    _check_rows(ref, got, what)
    assert torch.equal(got["sx"].reshape(B, n), d.reshape(1, n).expand(B, n)), what + " sx"
    assert torch.equal(got["zx"].reshape(B, n), (z.int() - cx).reshape(1, n).expand(B, n)), what + " zx"
    code = got["xq"][:, :C].int().reshape(B, n, C) + cx

    def quant(h):
        return fq.static_act_quant(qr.smoothed(h, s), d.reshape(1, n, 1), z.reshape(1, n, 1), ref.n_bits)[0].int()

    a, b = quant((ref.u64 - ref.m_u).half()), quant((ref.u64 + ref.m_u).half())
    bad = ~((code >= torch.minimum(a, b)) & (code <= torch.maximum(a, b)))           # (a smoothing entry may be negative)
    assert not bool(bad.any()), "%s codes: %s" % (what, _where(bad))
    shares = {}
    if got.get("xm") is not None:
        shares["xm"] = check_xm(ref, got["xm"], what)
        own = quant(got["xm"].reshape(B, n, C))
        bad = code != own
        assert not bool(bad.any()), "%s: codes are not the quantizer of the kernel's own xm: %s" % (what, _where(bad))
    return shares


def static_launch_of(u, smooth, deltas, zps, n_bits, C, want_xm=True):
    """What a correct static-arm kernel writes for the modulated activation u (fp32): one dict per output."""
    B, n, _ = u.shape
    cx = 128 if n_bits == 8 else 0
    h = u.half()
    outs = []
    for s, d, z in zip(smooth, deltas, zps):
        dd = d.reshape(-1).expand(n) if d.numel() == 1 else d.reshape(-1)
        zz = z.reshape(-1).expand(n) if z.numel() == 1 else z.reshape(-1)
        codes = fq.static_act_quant(qr.smoothed(h, s), dd.reshape(1, n, 1), zz.reshape(1, n, 1), n_bits)[0].int()
        xq = torch.zeros(B * n, (C + 127) // 128 * 128, dtype=torch.int8)
        xq[:, :C] = (codes - cx).reshape(B * n, C).to(torch.int8)
        zx = (zz.int() - cx).reshape(1, n).expand(B, n).reshape(-1).contiguous()
        outs.append({"xq": xq, "sx": dd.reshape(1, n).expand(B, n).reshape(-1).contiguous(), "zx": zx,
                     "R": (xq.int().sum(-1) - C * zx).int(), "status": 0, "xm": h if want_xm else None})
    return outs
