"""cross_attn.q_linear + cross attention: the two-launch route (vq_gemm_i8 into a dense q, then vq_attn_fwd) against the
fused entry point vq_gemm_i8_cross_attn, at the cross-attention shapes of STDiT-XL/2 and PixArt (GPU only).

Captured graphs replayed, the activation codes rotated over 12 buffers so that no launch finds its input in L2 / MALL (the
weight and the prompt's K | V stay, as they do in a step), the two routes alternated three times in one process after a
warm-up.  Bytes are the algorithm's: both routes read M K + N K (/ 2 for nibble weights) and the prompt's K | V and write
att_o (M N 2); the two-launch route also writes and reads q (M N 2 each way).  The rule of the route: fused
stays default-on at a shape only where it is faster than the pair in ALL three alternations.

    python tools/cross_q_fused_time.py [--out profiles/cross_q_fused/kernel_times.json] [--no-resources]

Also prints the VGPR / SGPR / scratch figures of the kernel (the source compiled to assembly with the build's flags) and
its dynamic LDS.  Exit status 1 when the fused launch loses an alternation at a shape the route takes (a shape the entry
point admits but the route's whole-round rule refuses is timed and reported all the same).
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import viditq_amd  # noqa: E402,F401
from static_quant_time import graph_time  # noqa: E402
from viditq_amd import build as vq_build  # noqa: E402
from viditq_amd import ops  # noqa: E402
from viditq_amd.t2v.stdit import _CROSS_Q_FUSED_ROUND, _cross_q_fused_shape  # noqa: E402

D, H, C = 72, 16, 1152
# (name, samples, tokens per sample, keys per sample, weight bits)
SHAPES = [("STDiT-XL/2 16x512x512, one sample (the benchmark)", 1, 16384, (120,), 8),
          ("STDiT-XL/2 16x512x512, W4", 1, 16384, (120,), 4),
          ("STDiT-XL/2 joint cond | uncond", 2, 16384, (120, 120), 8),
          ("PixArt-alpha 512, uncond | cond", 2, 1024, (120, 77), 8),
          ("PixArt-Sigma 1024, uncond | cond, 180 live keys", 2, 4096, (180, 180), 4)]
LDS_BYTES = 8 * 64 * (144 * 2 + 16) + 16 * 288 + 12 * 256         # WideCfg<256, 288, 4, 2>::LDS: slabs + parameter blocks


def kernel_resources():
    """{kernel: {vgpr, sgpr, scratch}} of the fused kernels: csrc/gemm_i8.hip compiled to assembly with the build's flags."""
    src = os.path.join(vq_build.CSRC, "gemm_i8.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "gemm_i8.s")
        subprocess.run([vq_build._hipcc(), *vq_build._flags("gemm_i8.hip"), "-Wno-inline-asm", "--offload-device-only", "-S", src,
                        "-o", out], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(out).read()
    res = {}
    for rec in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", rec)
        if not name or "gemm_i8_cross_attn_kernel" not in name.group(1):
            continue
        f = {k: int(re.search(r"\.%s:\s+(\d+)" % k, rec).group(1)) for k in
             ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")}
        res["W4" if "ILb1E" in name.group(1) else "W8"] = dict(
            vgpr=f["vgpr_count"], sgpr=f["sgpr_count"], scratch_bytes=f["private_segment_fixed_size"],
            vgpr_spills=f["vgpr_spill_count"], sgpr_spills=f["sgpr_spill_count"], dynamic_lds_bytes=LDS_BYTES)
    return res


def operands(B, Nt, lens, bits, dev):
    """12 activations of per-token codes, one packed weight and the samples' K | V."""
    M = B * Nt
    acts = [ops.rowquant(torch.randn(1, M, C, device=dev).half(), n_bits=8) for _ in range(12)]
    W = (torch.randn(C, C, device=dev) * C ** -0.5).half()
    pw = ops.pack_weight(W, *ops.weight_minmax(W, bits), bits)
    bias = (torch.randn(C, device=dev) * 0.3).float()
    kv = torch.randn(sum(lens), 2 * C, device=dev).half()
    offs = torch.tensor([0] + [sum(lens[:i + 1]) for i in range(B)], dtype=torch.int32, device=dev)
    return acts, pw, bias, kv, offs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-resources", action="store_true", help="skip the compile that reads the kernel's register figures")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cross_q_fused_time.py needs a GPU: a CPU run gives no time")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = {} if args.no_resources else kernel_resources()
    for k, v in res.items():
        print("gemm_i8_cross_attn_kernel %s: %s" % (k, v), flush=True)
    rows_out = []
    for name, B, Nt, lens, bits in SHAPES:
        M, bound = B * Nt, max(lens)
        takes = _cross_q_fused_shape(H, D, C, B, Nt, bound)                       # the entry point's contract
        routed = takes and ((M // 256) * (C // 288)) % _CROSS_Q_FUSED_ROUND == 0   # ... and the route's whole-round rule
        acts, pw, bias, kv, offs = operands(B, Nt, lens, bits, dev)
        q = torch.empty((M, C), dtype=torch.float16, device=dev)
        o2, of = torch.empty_like(q), torch.empty_like(q)
        i = [0]

        def act():
            i[0] = (i[0] + 1) % len(acts)
            return acts[i[0]]

        def two(a=None):
            ops.gemm_i8(a or act(), pw, bias=bias, out=q)
            return ops.attn_fwd(q, kv, kv[:, C:], o2, B, Nt, bound, H, D, Nt * C, C, 0, kv.stride(0), Nt * C, C, kv_off=offs)

        def fused(a=None):
            return ops.gemm_i8_cross_attn(a or act(), pw, bias, kv, kv[:, C:], of, B, Nt, bound, H, D, 0, kv.stride(0), Nt * C, C,
                                          kv_off=offs)

        mb_fused = (M * C + C * C // (2 if bits <= 4 else 1) + kv.numel() * 2 + M * C * 2) / 1e6
        mb_two = mb_fused + 2 * M * C * 2 / 1e6
        if not takes:
            t_two = [graph_time(two)[0] for _ in range(3)]
            rows_out.append(dict(shape=name, route="refused by the shape contract (keys > 128): the pair stays",
                                 two_launch_MB=round(mb_two, 1), two_launch_us=[round(t, 1) for t in t_two]))
            print("%-52s refused by the contract; two launches %s" % (name, ["%.1f" % t for t in t_two]), flush=True)
            continue
        assert torch.equal(two(acts[0]), fused(acts[0])), "routes disagree"
        t_two, t_fused = [], []
        keep = [graph_time(two)[1], graph_time(fused)[1]]            # warm-up of both routes
        for _ in range(3):
            t_two.append(graph_time(two)[0])
            t_fused.append(graph_time(fused)[0])
        del keep
        wins = all(f < t for f, t in zip(t_fused, t_two)) and max(t_fused) < min(t_two)
        rows_out.append(dict(shape=name, two_launch_MB=round(mb_two, 1), fused_MB=round(mb_fused, 1),
                             two_launch_us=[round(t, 1) for t in t_two], fused_us=[round(t, 1) for t in t_fused],
                             fused_faster_in_all_three=wins, route_takes_it=routed))
        print("%-52s two launches %s | fused %s | %s; the route %s" % (
            name, ["%.1f" % t for t in t_two], ["%.1f" % t for t in t_fused],
            "fused faster in all three" if wins else "FUSED LOSES", "takes it" if routed else "refuses it"), flush=True)
        del acts, pw
        torch.cuda.empty_cache()
    rec = dict(device=torch.cuda.get_device_name(0), kernel_resources=res, shapes=rows_out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0 if all(r["fused_faster_in_all_three"] for r in rows_out if r.get("route_takes_it")) else 1


if __name__ == "__main__":
    sys.exit(main())
