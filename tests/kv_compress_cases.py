"""Inputs, the float64 reference and the per-element bounds of tests/test_kv_compress_gpu.py (ops.kv_compress)."""
import torch
import torch.nn.functional as F

SHAPES = [(2, 4, 6, 2), (1, 8, 4, 4)]          # (B, H, W, sr): non-square, B = 2 for the sequence stride
EPS = 1e-5                                     # nn.LayerNorm's default
# The fp32 evaluation term of the tight bound, in fp16 ulps at the reference value.  Measured on the CPU: reference()
# in float32 against float64 on every arithmetic case of the GPU test (k', v' and q; seeds 0-2) misses the half-ulp by at
# most 0.0002 ulp; the term is twice that.  The same run: no float32 element outside the loose bound or the tight one.
FP32_TERM = 0.0004


def make(B, H, W, sr, C, qk_norm, seed=0):
    """The q | k | v buffer [B*H*W (+ one NaN guard row), 3C] fp16 with a per-channel offset of a few units, and non-trivial
    fp32 parameters.  Without qk_norm the q columns are NaN: the kernel must not touch them."""
    g = torch.Generator().manual_seed(1000 * seed + 16 * C + sr)
    r = lambda *s: torch.randn(*s, generator=g)
    buf = (r(B * H * W + 1, 3 * C) + 3.0 * r(3 * C)).half()
    buf[-1] = float("nan")
    if not qk_norm:
        buf[:, :C] = float("nan")
    # LayerNorm biases of +-6: no output near zero, where an fp16 ulp is finer than fp32 arithmetic on O(1) operands
    ln = lambda: (1.0 + 0.3 * r(C), torch.sign(r(C)) * (6.0 + 0.3 * r(C)), EPS)
    return dict(buf=buf, sr_w=0.25 + 0.15 * r(C, 1, sr, sr), sr_b=r(C), norm=ln(), k_norm=ln() if qk_norm else None,
                q_norm=ln() if qk_norm else None)


def _ln(x, p, dt):
    return F.layer_norm(x, x.shape[-1:], p[0].to(dt), p[1].to(dt), p[2])


def reference(d, B, H, W, sr, C, sampling, dt=torch.float64):
    """-> (q rows [B*N, C] or None, k', v', all unrounded in ``dt``, loose-bound extra of k' or None): the expressions of
    oracle/pixart_ref.kv_downsample and F.layer_norm in ``dt``, .half() after k_norm / q_norm (and at the end, by the caller).
    The extra: one fp16 ulp of an intermediate (k_norm) value through the conv weight and the final LayerNorm's rstd * weight."""
    N = H * W
    x = d["buf"][:B * N].to(dt)
    q = _ln(x[:, :C], d["q_norm"], dt) if d["q_norm"] else None
    k, v = x[:, C:2 * C].reshape(B, N, C), x[:, 2 * C:].reshape(B, N, C)
    if d["k_norm"]:
        k = _ln(k, d["k_norm"], dt)
        if sampling == "conv":                     # (a pick commutes with the rounding: its reference stays unrounded)
            k = k.half().to(dt)

    def down(t):
        if sampling == "uniform_every":
            return t[:, ::sr], None
        gr = t.reshape(B, H, W, C).permute(0, 3, 1, 2)
        if sampling in ("uniform", "ave"):
            return gr[:, :, ::sr, ::sr].permute(0, 2, 3, 1).reshape(B, -1, C), None
        w = d["sr_w"].to(dt)
        s = F.conv2d(gr, w, d["sr_b"].to(dt), stride=sr, groups=C).reshape(B, C, -1).permute(0, 2, 1)
        u = _tap_ulp(gr, w, sr)
        rstd = (s.var(-1, unbiased=False, keepdim=True) + EPS).rsqrt()
        return _ln(s, d["norm"], dt), u.reshape(B, C, -1).permute(0, 2, 1) * rstd * d["norm"][0].to(dt).abs()
    (k2, extra), (v2, _) = down(k), down(v)
    return q, k2.reshape(-1, C), v2.reshape(-1, C), (extra.reshape(-1, C) if extra is not None and d["k_norm"] else None)


def _tap_ulp(gr, w, sr):
    """[B, C, H/sr, W/sr]: max over the sr x sr window of |w[c, di, dj]| * ulp16(gr[b, c, i sr + di, j sr + dj])."""
    B, C, H, W = gr.shape
    t = ulp16(gr).reshape(B, C, H // sr, sr, W // sr, sr) * w.abs().reshape(1, C, 1, sr, 1, sr)
    return t.amax(dim=(3, 5))


def ulp16(y):
    """The fp16 spacing at |y| (float64; 2^-24 below the smallest normal)."""
    e = torch.floor(torch.log2(y.abs().double().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10)


def check(got, ref, extra, arithmetic):
    """``got`` fp16 against the unrounded ``ref``: bit-equal for a copy; else no element outside the loose bound (the
    result is one of ref's two fp16 neighbours - an fp32 evaluation is far finer than an fp16 ulp - plus, behind k_norm
    and the convolution, ``extra``) and at most 1 in 1000 outside the tight one (half an ulp + FP32_TERM)."""
    if not arithmetic:
        assert torch.equal(got, ref.half())
        return 0.0
    err = (got.double() - ref.double()).abs()
    assert torch.isfinite(got).all()
    if extra is None:
        loose = ulp16(ref)
    else:
        loose = (0.5 + FP32_TERM) * ulp16(ref.abs() + extra) + extra
    tight = (0.5 + FP32_TERM) * ulp16(ref)
    worst = ((err - 0.5 * ulp16(ref)) / ulp16(ref)).max().item()
    n_out = int((err > tight).sum())
    print("excess over half an ulp %.4f ulp; %d of %d outside the tight bound" % (worst, n_out, err.numel()))
    assert (err <= loose).all(), ((err - loose).max().item(), worst)
    assert n_out <= err.numel() / 1000, (n_out, err.numel(), worst)
    return worst
