"""The patch-major PixArt steps without a GPU: the three symbols against the header, the refusal table and its order against
the ``*_ok`` predicates, and forward(patch_major=True) of the tiny PixArt against the default forward."""
import ctypes
import os
import re

import pytest
import torch

from helpers import _FakeTensor, load_npz, state_dict_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = 1 << 20
PTRS = {"dpmpp": ("eps", "x", "hist", "coef", "step", "x_out", "x_model"),
        "ddpm": ("eps", "x", "noise", "coef", "step", "x_out", "x0_out", "x_model"),
        "sa": ("eps", "x", "xp", "hist", "noise", "coef", "step", "x_out", "xp_out", "x_model")}
BASE = dict(n=1, C=4, C_out=8, H=4, W=6, p=2, ld_eps=192, guided=3, row=0, n_rows=1, eps_f16=0, xm_f16=0, stream=None)
# (arguments on top of the valid base, the code the entry point must return); none of them reaches a HIP call
REFUSALS = [
    (dict(eps=None), -1), (dict(x=None), -1), (dict(coef=None), -1), (dict(x_out=None), -1), (dict(n=0), -1), (dict(C=0), -1),
    (dict(C_out=0), -1), (dict(H=0), -1), (dict(W=-6), -1), (dict(p=0), -1), (dict(row=-1), -1), (dict(row=1), -1),
    (dict(n_rows=0), -1),
    (dict(C=9), -2), (dict(H=5), -2), (dict(W=7), -2), (dict(ld_eps=191), -2),               # C > C_out, H % p, W % p, the pitch
    (dict(n=65536), -2), (dict(H=2 * 65536, ld_eps=2 * 65536 * 6 * 8), -2),                  # grid extents
    (dict(eps=GOOD + 2), -2), (dict(eps=GOOD + 1, eps_f16=1), -2), (dict(x=GOOD + 2), -2), (dict(x_out=GOOD + 1), -2),
    (dict(x_model=GOOD + 2), -2), (dict(x_model=GOOD + 1, xm_f16=1), -2), (dict(step=GOOD + 2), -2), (dict(coef=GOOD + 2), -2),
    (dict(H=8, W=8, p=4, ld_eps=512), -4), (dict(H=6, p=3, ld_eps=288), -4), (dict(eps_f16=2), -4), (dict(eps_f16=-1), -4),
    (dict(xm_f16=3), -4),
    # the order: EINVAL before ESHAPE before EUNSUP
    (dict(eps=None, ld_eps=191, eps_f16=2), -1), (dict(row=-1, H=6, p=3), -1), (dict(ld_eps=191, eps_f16=2), -2),
    (dict(x=GOOD + 2, xm_f16=3), -2), (dict(H=5, eps_f16=2), -2)]
ONLY = {"dpmpp": [(dict(hist=None), -1)],
        "ddpm": [(dict(noise=None), -1), (dict(guided=-1), -1), (dict(guided=5), -2), (dict(C=5), -2),       # 2C > C_out
                 (dict(guided=-1, H=5), -1), (dict(guided=5, eps_f16=2), -2)],
        "sa": [(dict(xp=None), -1), (dict(hist=None), -1), (dict(noise=None), -1), (dict(xp_out=None), -1)]}
# accepted: the wide form, and what selects the one-element form instead of a refusal
VALID = [dict(), dict(eps_f16=1), dict(ld_eps=200), dict(ld_eps=193), dict(eps=GOOD + 4), dict(eps=GOOD + 2, eps_f16=1),
         dict(x=GOOD + 4), dict(C=3, C_out=6, ld_eps=144), dict(C_out=10, ld_eps=240), dict(W=5, p=1, ld_eps=160), dict(n=3),
         dict(H=6, W=4)]


def _names(kind):
    tail = ["n", "C", "C_out", "H", "W", "p", "ld_eps", "guided", "row", "n_rows", "eps_f16", "xm_f16", "stream"]
    return list(PTRS[kind]) + [t for t in tail if t != "guided" or kind == "ddpm"]


def _args(kind, **kw):
    a = dict({k: None if k in ("step", "x0_out", "x_model") else GOOD for k in PTRS[kind]}, **BASE)
    assert set(kw) <= set(a)
    a.update(kw)
    return [ctypes.c_void_p(a[k]) if k in PTRS[kind] and a[k] is not None else a[k] for k in _names(kind)]


def _fakes(kw):
    a = dict(BASE, eps=GOOD, x=GOOD)
    a.update(kw)
    n, C, H, W, p, cols = a["n"], a["C"], a["H"], a["W"], a["p"], a["p"] ** 2 * a["C_out"]
    dt = {0: torch.float32, 1: torch.float16}.get(a["eps_f16"], torch.bfloat16)
    return (_FakeTensor((2 * n, H * W // (p * p), cols), (a["ld_eps"], cols, 1), a["eps"], dt),
            _FakeTensor((n, C, H, W), (C * H * W, H * W, W, 1), a["x"], torch.float32))


@pytest.mark.parametrize("kind", sorted(PTRS))
def test_symbol_refusal_table_its_order_and_the_ok_predicate(kind):
    """vq_cfg_<kind>_step_patch2d is declared in the header with the binding's signature; it returns the table's code before
    any HIP call; ops.cfg_<kind>_step_patch2d_ok says no exactly where it refuses on what the predicate is given (eps, x)
    and yes on the accepted layouts."""
    import __graft_entry__ as ge
    ge.build()
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib, ops
    name = "vq_cfg_%s_step_patch2d" % kind
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "viditq.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, src, flags=re.S)
    assert m, "%s is not declared in include/viditq.h" % name
    params = [" ".join(q.split()) for q in m.group(1).split(",")]
    assert [re.search(r"(\w+)$", q).group(1) for q in params] == _names(kind)
    kinds = [ctypes.c_void_p if "*" in q else (ctypes.c_long if q.startswith("long") else ctypes.c_int) for q in params]
    assert _lib.SIGNATURES[name] == (ctypes.c_int, kinds)
    fn, ok = getattr(_lib.load(), name), getattr(ops, "cfg_%s_step_patch2d_ok" % kind)
    given, asked = {"eps", "x", "n", "C", "C_out", "H", "W", "p", "ld_eps", "eps_f16"}, 0
    for kw, code in REFUSALS + ONLY[kind]:
        assert fn(*_args(kind, **kw)) == code, kw
        if set(kw) <= given and None not in kw.values() and min(list(kw.values()) + [0]) >= 0 and kw.get("p", 2) > 0:
            assert ok(*_fakes(kw)) is False, kw
            asked += 1
    assert asked >= 12
    for kw in VALID:
        assert ok(*_fakes(kw)) is True, kw
        assert fn(*_args(kind, **dict(kw, row=-1))) == -1, kw                 # only the row is wrong
        assert fn(*_args(kind, **dict(kw, xm_f16=3))) == -4, kw               # ... or only a flag: the last check
    for attr, val in (("dtype", torch.float16), ("is_cuda", False)):          # the latent is fp32; GPU tensors
        eps, x = _fakes({})
        setattr(x, attr, val)
        assert ok(eps, x) is False
    eps, x = _fakes({})
    eps._st = (192, 40, 1)
    assert ok(eps, x) is False                                                # a sample is dense
    with pytest.raises(ops.VQError):
        getattr(ops, "cfg_%s_step_patch2d" % kind)(*[torch.zeros(2, 6, 32)] + [torch.zeros(1, 4, 4, 6)] * 6)


@pytest.mark.parametrize("net", ["PixArt", "PixArtMS"])
def test_patch_major_forward_unpatchified_is_the_default_forward(net):
    """The tiny PixArt of tests/golden on the CPU in fp32, without its blocks (their attention is a HIP kernel; the flag
    acts behind final_layer, and tests/test_t2i_patch_major_gpu.py runs the whole net): forward(patch_major=True) is
    final_layer's [B, h*w, p*p*C_out], unpatchify of it equals forward() exactly, forward_with_dpmsolver / forward_with_cfg
    hand it on untouched, and the default results have not moved."""
    import viditq_amd  # noqa: F401
    from viditq_amd import t2i
    g = load_npz("tiny_pixart_w8a8.npz")
    m = getattr(t2i, net)(input_size=16, depth=0, hidden_size=64, num_heads=4, model_max_length=12, caption_channels=32)
    have = m.state_dict()
    m.load_state_dict({k: v for k, v in state_dict_of(g).items() if k in have and v.shape == have[k].shape}, strict=False)
    torch.manual_seed(0)
    torch.nn.init.normal_(m.final_layer.linear.weight, std=0.05)             # (zero-initialised: every output would be 0)
    m = m.float().eval()
    H, W = (16, 16) if net == "PixArt" else (8, 24)                          # PixArtMS: a non-square grid
    x, t = torch.randn(2, 4, H, W), torch.tensor([500.0, 500.0])
    y, mask = g["y"][:1].float().repeat(2, 1, 1, 1), g["mask"][:1].repeat(2, 1)
    with torch.no_grad():
        want = m.forward(x, t, y, mask)
        pm = m.forward(x, t, y, mask, patch_major=True)
        assert (m.h, m.w) == (H // 2, W // 2) and tuple(pm.shape) == (2, H * W // 4, 4 * 8) and float(pm.abs().max()) > 0
        assert torch.equal(m.unpatchify(pm), want) and tuple(want.shape) == (2, 8, H, W)
        assert torch.equal(m.forward_with_dpmsolver(x, t, y, mask=mask, patch_major=True), pm)
        assert torch.equal(m.forward_with_dpmsolver(x, t, y, mask=mask), want.chunk(2, dim=1)[0])
        x2 = x[[0, 0]]
        assert torch.equal(m.forward_with_cfg(x, t, y, 4.5, mask, patch_major=True), m.forward(x2, t, y, mask, patch_major=True))
        assert torch.equal(m.forward_with_cfg(x, t, y, 4.5, mask), m.guide_cfg(m.forward(x2, t, y, mask), 4.5))
