"""Round 6: attention kernels timed from graph replays (GPU box only).  One process = one arm: VIDITQ_LIB selects another
build of the same C ABI, --lab-kernel=<id> a retired spatial / image kernel of tools/lab/attn_lab.hip (ids in tools/lab/lab.py);
run it alternately over the arms from a shell loop.  Prints one line per shape:
spatial 16 x 1024 (STDiT), image 2 x 4096 (PixArt-Sigma, B = 2), cross 16384 x 120, temporal + quantizer 1024 x 16; only when
named: "short" (64 x 160 queries x 1024 keys, the four-wave attn_fwd8_kernel), "temporal8" (temporal + quantizer with 8 heads:
attn_temporal_quant_kernel) and "temporal_wide" (16 heads with code rows of Kp = 2176: the same kernel, through the C ABI).
--dump=<file> / --cmp=<file> save / compare outputs instead of timing: of the vq_attn_fwd kernels, of the temporal kernels with a
fused quantizer ("temporal" named alone), or of both (no name)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viditq_amd  # noqa
from viditq_amd import ops, _lib

dev = torch.device("cuda:0")
H, D = 16, 72
g = torch.Generator().manual_seed(0)
LAB_KERNEL = next((int(w[13:]) for w in sys.argv[1:] if w.startswith("--lab-kernel=")), None)
WHICH = [w for w in sys.argv[1:] if not w.startswith("--lab-kernel=")] or ["spatial", "image", "cross", "temporal"]
if LAB_KERNEL is None:
    self_attn = ops.attn_fwd
else:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "lab"))
    import lab  # noqa: E402

    def self_attn(*a):
        return lab.attn_fwd(LAB_KERNEL, *a)


def timeit(fn, n=8, reps=10):
    fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        with torch.cuda.graph(gr, stream=st):
            for _ in range(n):
                fn()
    for _ in range(12):
        gr.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        gr.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (n * reps) * 1e3


tag = os.path.basename(os.path.dirname(_lib.LIB_PATH)) if LAB_KERNEL is None else "lab kernel %d" % LAB_KERNEL
out = []
# --dump=<file> / --cmp=<file>: outputs of fixed inputs, saved by one library and compared bit for bit by another - the three
# D = 72 self-attention shapes and every vq_attn_fwd entry of tests/attn_regimes._SHAPES (every route x head dim the suite
# knows) under R2 rising with the case's own step and lead, so that both the taken and the deferred rescale run
DUMP = next((w[7:] for w in WHICH if w.startswith("--dump=")), None)
CMP = next((w[6:] for w in WHICH if w.startswith("--cmp=")), None)
NAMED = [w for w in WHICH if not w.startswith("--")]


def regime_cases():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import attn_regimes as ar
    seen = set()
    for case in ar.cases():
        if case["kernel"].startswith("VQ_ATTN_K_") and case["regime"][0] == "R2" and not case["regime"][3] and \
                case["scale"] == case["D"] ** -0.5 and case["id"] not in seen:
            seen.add(case["id"])
            yield ar, case


def run_regime_case(ar, case):
    """The launch of tests/test_attention_softmax_gpu.py::_run_fwd; None when the K / V buffer cannot be allocated."""
    sh, D, scale = case["shape"], case["D"], case["scale"]
    n, Lq, lens, H = sh["n"], sh["Lq"], sh["lens"], sh["H"]
    Cc, a = H * D, ar.fwd_layout(case)
    q, k, v, _ = ar.build(case["regime"], n, Lq, lens, H, D, scale, case["seed"])
    big = a["kv_rows"] * a["kv_tok"] * 2 >= 1 << 30            # only the 2 GiB buffer of the FWD8_NW8 entry may be skipped
    try:
        if a["offs"] is not None:
            kvd = torch.cat([torch.cat([k[i, :L].reshape(L, Cc), v[i, :L].reshape(L, Cc)], 1) for i, L in enumerate(lens)]).to(dev)
            off = torch.tensor(a["offs"], dtype=torch.int32, device=dev)
        else:
            kvd = torch.zeros((a["kv_rows"], a["kv_tok"]), dtype=torch.float16, device=dev)
            kvd[:, :Cc] = k.reshape(n * lens[0], Cc).to(dev)
            kvd[:, Cc:2 * Cc] = v.reshape(n * lens[0], Cc).to(dev)
            off = None
    except torch.cuda.OutOfMemoryError:
        if not big:
            raise
        return None
    o = torch.full((n * Lq, Cc), float("nan"), dtype=torch.float16, device=dev)
    if LAB_KERNEL is None:                                     # the case runs the kernel its id names
        largs = (a["n_seq"], Lq, a["Lk"], H, D, a["q_seq"], a["q_tok"], a["kv_seq"], a["kv_tok"], a["o_seq"], a["o_tok"])
        route = _lib.load().vq_attn_fwd_route(o.data_ptr(), kvd.data_ptr(), kvd.data_ptr(), o.data_ptr(), *largs,
                                              None if off is None else off.data_ptr(), scale, None)
        assert route == ar.kernel_ids()[case["kernel"]], (case["id"], route)
    self_attn(q.reshape(n * Lq, Cc).to(dev), kvd, kvd[:, Cc:], o, a["n_seq"], Lq, a["Lk"], H, D, a["q_seq"], a["q_tok"], a["kv_seq"],
              a["kv_tok"], a["o_seq"], a["o_tok"], off, scale)
    return o.cpu()


def temporal_outputs():
    """{case: tensor} of every attn_temporal_quant / _quant2 / _long entry of tests/attn_regimes._SHAPES under R2 rising with the
    case's own step and lead, through the C ABI: the dynamic quantizer without and with a smoothing vector (fp16 copy included),
    the static one at 8 and 6 bits without and with it at B = 1 and B = 2 (delta = 2 / qmax, zp = round(qmax / 2)), the long
    kernel's plain fp16 form, and every H = 16 case again with code rows of Kp = 2176 (T <= 16: attn_temporal_quant_kernel
    instead of the trimmed one).  Per form: xq (pad columns included), sx, zx, R, o and the status word."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import attn_regimes as ar
    L = _lib.load()
    res, seen = {}, set()

    def p(t):
        return None if t is None else t.data_ptr()
    for case in ar.cases():
        if case["kernel"] not in ("attn_temporal_quant", "attn_temporal_quant2", "attn_temporal_long") or case["id"] in seen or \
                case["regime"][0] != "R2" or case["regime"][3] or case["scale"] != case["D"] ** -0.5:
            continue
        seen.add(case["id"])
        sh, D, scale = case["shape"], case["D"], case["scale"]
        T, S, Hh = sh["T"], sh["S"], sh["H"]
        Cc = Hh * D
        is_long = case["kernel"] == "attn_temporal_long"
        sm = torch.exp(torch.randn(Cc, generator=torch.Generator().manual_seed(3)) * 0.6).float().to(dev)
        sm_rcp = ops.smooth_rcp(sm)
        assert sm_rcp is not None
        for B in (1, 2):
            n, rows = B * S, B * T * S
            q, k, v, _ = ar.build(case["regime"], n, T, [T] * n, Hh, D, scale, case["seed"])
            qkv = torch.cat([x.reshape(B, S, T, Cc).permute(0, 2, 1, 3).reshape(rows, Cc) for x in (q, k, v)], 1).to(dev)
            qp, kp_, vp = qkv.data_ptr(), qkv[:, Cc:].data_ptr(), qkv[:, 2 * Cc:].data_ptr()
            for Kp in [(Cc + 127) // 128 * 128] + ([2176] if Hh == 16 else []):
                def outs():
                    return dict(xq=torch.full((rows, Kp), 77, dtype=torch.int8, device=dev), sx=torch.zeros(rows, device=dev),
                                zx=torch.zeros(rows, dtype=torch.int32, device=dev), R=torch.zeros(rows, dtype=torch.int32, device=dev),
                                o=torch.full((rows, Cc), float("nan"), dtype=torch.float16, device=dev),
                                status=torch.zeros(1, dtype=torch.int32, device=dev))

                def keep(form, t):
                    torch.cuda.synchronize()
                    for f, x in t.items():
                        res["%s|B%d|Kp%d|%s|%s" % (case["id"], B, Kp, form, f)] = x.cpu()
                for s_, r_, sn in ((None, None, "plain"), (sm, sm_rcp, "smooth")):
                    if B == 1:                     # per-token grids are shared over the batch: B = 1 only
                        t = outs()
                        if is_long:
                            _lib.check(L.vq_attn_temporal_long(qp, kp_, vp, p(s_), p(r_), p(t["xq"]), p(t["sx"]), p(t["zx"]), p(t["R"]),
                                                               p(t["status"]), p(t["o"]), B, T, S, Hh, D, 3 * Cc, Cc, Kp, scale, None))
                        else:
                            _lib.check(L.vq_attn_temporal_rowquant(qp, kp_, vp, p(s_), p(r_), p(t["xq"]), p(t["sx"]), p(t["zx"]),
                                                                   p(t["R"]), p(t["status"]), p(t["o"]), B, T, S, Hh, D, 3 * Cc, Kp,
                                                                   scale, None))
                        keep("dynamic-" + sn, t)
                    for n_bits in (8, 6):
                        qmax = 2 ** n_bits - 1
                        delta = torch.tensor([2.0 / qmax], device=dev)
                        zp = torch.tensor([float(round(qmax / 2))], device=dev)
                        t = outs()
                        del t["status"]
                        _lib.check(L.vq_attn_temporal_rowquant_static(qp, kp_, vp, p(s_), p(r_), p(delta), p(zp), p(t["xq"]), p(t["sx"]),
                                                                      p(t["zx"]), p(t["R"]), p(t["o"]), B, T, S, Hh, D, 3 * Cc, Cc, Kp,
                                                                      n_bits, scale, None))
                        keep("static%d-%s" % (n_bits, sn), t)
            if is_long:
                o = torch.full((rows, Cc), float("nan"), dtype=torch.float16, device=dev)
                _lib.check(L.vq_attn_temporal_long(qp, kp_, vp, None, None, None, None, None, None, None, p(o), B, T, S, Hh, D, 3 * Cc,
                                                   Cc, 0, scale, None))
                torch.cuda.synchronize()
                res["%s|B%d|fp16|o" % (case["id"], B)] = o.cpu()
    return res


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int16) if a.dtype == torch.float16 else
                                              a.view(torch.int32) if a.dtype == torch.float32 else a,
                                              b.view(torch.int16) if b.dtype == torch.float16 else
                                              b.view(torch.int32) if b.dtype == torch.float32 else b)


if DUMP or CMP:
    res = temporal_outputs() if not NAMED or "temporal" in NAMED else {}
    for name, n_seq, L in (("spatial", 16, 1024), ("image", 2, 4096), ("ragged", 3, 1000)) if NAMED != ["temporal"] else ():
        M = n_seq * L
        q = (torch.randn(M, 3 * 1152, generator=torch.Generator().manual_seed(7)) * 1.3).half().to(dev)
        o = torch.zeros((M, 1152), dtype=torch.float16, device=dev)
        self_attn(q, q[:, 1152:], q[:, 2304:], o, n_seq, L, L, H, D, L * 3456, 3456, L * 3456, 3456, L * 1152, 1152)
        res[name] = o.cpu()
    for ar, case in regime_cases() if NAMED != ["temporal"] else ():
        out_ = run_regime_case(ar, case)
        if out_ is None:
            print("%-16s skipped %s: its K / V buffer could not be allocated" % (tag, case["id"]))
        else:
            res[case["id"]] = out_
    if DUMP:
        torch.save(res, DUMP)
        print("%-16s dumped %d cases to %s" % (tag, len(res), DUMP))
    else:
        ref = torch.load(CMP)
        def where(a, b):                                       # how many elements differ, and the first of them
            if a.shape != b.shape:
                return "shapes %s / %s" % (tuple(a.shape), tuple(b.shape))
            ne = (a != b) & ~((a != a) & (b != b))
            return "%d differ, first at %s" % (int(ne.sum()), tuple(int(x) for x in ne.nonzero()[0]) if bool(ne.any()) else "-")
        lines = ["%s %s (max |d| %.3g)" % (k, "bit-identical" if same_bits(res[k], ref[k]) else "DIFFERS: " + where(res[k], ref[k]),
                                           float((res[k].float() - ref[k].float()).abs().nan_to_num(0.0).max())) if k in ref
                 else "%s NOT IN DUMP" % k for k in res]
        lines += ["%s ONLY IN DUMP" % k for k in ref if k not in res]
        print("%-16s vs %s:\n  %s" % (tag, CMP, "\n  ".join(lines)))
        print("%d cases, %d bit-identical" % (len(lines), sum(ln.endswith(")") and " bit-identical " in ln for ln in lines)))
        sys.exit(0 if all(" bit-identical " in ln for ln in lines) else 1)
    sys.exit(0)
# "short" (only when named): 160 queries per sequence against 1024 keys - the four-wave attn_fwd8_kernel (VQ_ATTN_K_FWD8_NW4)
for name, n_seq, L, Lq in (("spatial", 16, 1024, 1024), ("image", 2, 4096, 4096), ("short", 64, 1024, 160)):
    if name not in WHICH or (name == "short" and "short" not in sys.argv[1:]):
        continue
    M = n_seq * L
    bufs = [torch.randn(M, 3 * 1152, generator=g).half().to(dev) for _ in range(3)]
    o = torch.empty((n_seq * Lq, 1152), dtype=torch.float16, device=dev)
    ld = 3456
    i = [0]

    def f():
        i[0] = (i[0] + 1) % len(bufs)
        q = bufs[i[0]]       # (Lq < L: the first Lq rows of every sequence are its queries)
        self_attn(q, q[:, 1152:], q[:, 2304:], o, n_seq, Lq, L, H, D, L * ld, ld, L * ld, ld, Lq * 1152, 1152)
    t = timeit(f)
    fl = 4.0 * n_seq * Lq * L * H * D
    out.append("%s %dx%dx%d %.1f us (%.0f TF)" % (name, n_seq, Lq, L, t, fl / t / 1e6))
if "cross" in WHICH:
    qs = [torch.randn(16384, 1152, generator=g).half().to(dev) for _ in range(3)]
    kv = torch.randn(120, 2304, generator=g).half().to(dev)
    off = torch.tensor([0, 120], dtype=torch.int32, device=dev)
    o = torch.empty_like(qs[0])
    i = [0]

    def f():
        i[0] = (i[0] + 1) % len(qs)
        # Lk = the bound on every sample's kv length, as QuantAttention.cross passes it (with Lk = 0 the dispatcher cannot
        # know the keys fit two tiles and takes the generic kernel: what this tool timed until round 6, call 20)
        ops.attn_fwd(qs[i[0]], kv, kv[:, 1152:], o, 1, 16384, 120, H, D, 16384 * 1152, 1152, 0, 2304, 16384 * 1152, 1152, kv_off=off)
    out.append("cross 16384x120 %.1f us" % timeit(f))
for name, Ht, Kp in (("temporal8", 8, 640), ("temporal_wide", 16, 2176)):        # (only when named) attn_temporal_quant_kernel
    if name not in WHICH:
        continue
    Ct = Ht * D
    qkvs = [torch.randn(16384, 3 * Ct, generator=g).half().to(dev) for _ in range(3)]
    xq, sx = torch.empty((16384, Kp), dtype=torch.int8, device=dev), torch.empty(16384, device=dev)
    zx, R = torch.empty(16384, dtype=torch.int32, device=dev), torch.empty(16384, dtype=torch.int32, device=dev)
    i = [0]

    def f():
        i[0] = (i[0] + 1) % len(qkvs)
        q = qkvs[i[0]]
        _lib.check(_lib.load().vq_attn_temporal_rowquant(
            q.data_ptr(), q[:, Ct:].data_ptr(), q[:, 2 * Ct:].data_ptr(), None, None, xq.data_ptr(), sx.data_ptr(), zx.data_ptr(),
            R.data_ptr(), None, None, 1, 16, 1024, Ht, D, 3 * Ct, Kp, D ** -0.5, torch.cuda.current_stream().cuda_stream))
    t = timeit(f)
    out.append("%s 1024x16 H=%d Kp=%d %.1f us (%.2f TB/s)" % (name, Ht, Kp, t, (16384 * 3 * Ct * 2 + 16384 * Kp) / t / 1e6))
if "temporal" in WHICH:
    qkvs = [torch.randn(16384, 3456, generator=g).half().to(dev) for _ in range(3)]
    i = [0]

    def f():
        i[0] = (i[0] + 1) % len(qkvs)
        q = qkvs[i[0]]
        ops.attn_temporal_rowquant(q, q[:, 1152:], q[:, 2304:], 1, 16, 1024, H, D, 3456)
    t = timeit(f)
    out.append("temporal+quant 1024x16 %.1f us (%.2f TB/s)" % (t, (16384 * 3456 * 2 + 16384 * 1152) / t / 1e6))
print("%-16s %s" % (tag, " | ".join(out)), flush=True)
