"""Two builds of the library against each other on the fused sampler steps, in ONE process (GPU box only):

    tools/sampler_step_ab.py OLD.so NEW.so

Both are loaded by path; vq_cfg_dpmpp_step and vq_cfg_ddpm_step of each get the same seeded inputs and every output
buffer (x_out, the history / pred_xstart, x_model) is compared byte for byte.  Shapes: those of tests/dpm_step_cases.py
and tests/ddpm_step_cases.py plus one PixArt 1024 x 1024 latent (1 x 4 x 128 x 128) and a batch of 80 of them, which the
capped grid of 1024 blocks walks in several passes; fp16 and fp32 model outputs, dense and padded pitch, no / fp16 / fp32
x_model, the row picked by the argument and by the device counter, rows of every order and solver type.  Prints one
JSON line; exit status 1 when any comparison differs.
"""
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viditq_amd  # noqa: E402,F401
from viditq_amd import _lib as L  # noqa: E402
from viditq_amd.t2i import IDDPM, DPMS_sigma  # noqa: E402

SHAPES = [(1, 4, 1), (2, 3, 7), (2, 4, 1024), (5, 4, 65536), (1, 3, 100003), (1, 4, 128 * 128), (80, 4, 128 * 128)]


def bind(path):
    lib = C.CDLL(os.path.abspath(path))
    for name in ("vq_cfg_dpmpp_step", "vq_cfg_ddpm_step"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = L.SIGNATURES[name]
    return lib


def same(a, b):
    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


def main(old_path, new_path):
    dev = torch.device("cuda:0")
    libs = [bind(old_path), bind(new_path)]
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    solver = DPMS_sigma(None, torch.zeros(1), torch.zeros(1), 4.5)
    dpm_rows = torch.cat([solver.multistep_rows(6, 3), solver.multistep_rows(6, 2, solver_type="taylor")]).to(dev)
    ddpm_rows = torch.cat([IDDPM("20").step_rows(4.5, False), IDDPM("10").step_rows(4.5, True)]).to(dev)
    g = torch.Generator(device=dev).manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev)   # noqa: E731
    compared = differing = 0
    for n, Cc, inner in SHAPES:
        CI, tot = Cc * inner, n * Cc * inner
        big = tot > 1 << 22
        x, z, hist0 = rnd(tot), rnd(tot), rnd(3 * tot)
        for mult, name, rows in ((1, "vq_cfg_dpmpp_step", dpm_rows), (2, "vq_cfg_ddpm_step", ddpm_rows)):
            for e16 in (1, 0):
                for pad in (0, 8):
                    ld = mult * CI + pad
                    eps = rnd(2 * n * ld).to(torch.float16 if e16 else torch.float32)
                    if mult == 2:                                       # variance channels in [-1.2, 1.2]
                        eps.view(2 * n, ld)[:, CI:2 * CI].clamp_(-1.2, 1.2)
                    for xm_dtype in (None, torch.float16, torch.float32):
                        picks = [(r, None) for r in range(rows.shape[0])] if not big and not pad and xm_dtype is None \
                            else [(1, None), (0, torch.full((1,), rows.shape[0] - 2, dtype=torch.int32, device=dev))]
                        for row, counter in picks:
                            outs = []
                            for lib in libs:
                                xo = torch.full((tot,), float("nan"), device=dev)
                                aux = hist0.clone() if mult == 1 else torch.full((tot,), float("nan"), device=dev)
                                xm = None if xm_dtype is None else torch.full((2 * tot,), float("nan"), dtype=xm_dtype,
                                                                              device=dev)
                                m16 = int(xm_dtype == torch.float16)
                                if mult == 1:
                                    rc = lib.vq_cfg_dpmpp_step(p(eps), p(x), p(aux), p(rows), p(counter), p(xo), p(xm), n, Cc,
                                                               inner, ld, row, rows.shape[0], e16, m16, stream)
                                else:
                                    rc = lib.vq_cfg_ddpm_step(p(eps), p(x), p(z), p(rows), p(counter), p(xo), p(aux), p(xm), n,
                                                              Cc, inner, ld, 3, row, rows.shape[0], e16, m16, stream)
                                assert rc == 0, (name, rc)
                                outs.append([xo, aux] + ([xm] if xm is not None else []))
                            torch.cuda.synchronize()
                            compared += len(outs[0])
                            if not same(*outs):
                                differing += 1
                                print("DIFFERS", name, (n, Cc, inner), dict(e16=e16, pad=pad, xm=str(xm_dtype), row=row,
                                                                            counter=counter is not None), flush=True)
    print(json.dumps({"old": old_path, "new": new_path, "buffers_compared": compared, "launch_pairs_differing": differing}))
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
