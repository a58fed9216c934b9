"""Record the launch traces of the fused block route (needs the GPU; reads nothing outside the repository).

Run:  python tests/golden/make_block_traces.py [--out FILE]        (writes tests/golden/fused_block_traces.json)

on a checkout of the commit whose launches are to be kept, with only the test-side files added (tests/helpers.py,
tests/block_trace_cases.py, this file).  Every case of block_trace_cases.CASES is built and run TWICE from scratch:
* the two ordered lists of ops calls (function, shape / dtype / strides of every tensor argument, value of every scalar
  argument; no addresses) must be equal - a list that depended on what ran before could not be pinned;
* the SHA-256 of the output bytes is stored where the two runs agree; where they do not, the case says
  ``"sha256": null`` and tests/test_block_trace_gpu.py compares its trace only.
The distinct call records are stored once (``calls``); a case's trace is a list of indices into them.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import block_trace_cases as bt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=bt.FIXTURE)
    args = ap.parse_args()
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib
    _lib.load()
    dev = torch.device("cuda:0")
    table, cases, bad = {}, {}, []
    for name in bt.NAMES:
        try:
            (calls, sha), (calls2, sha2) = bt.run_case(name, dev), bt.run_case(name, dev)
        except Exception as e:                               # (reported; the other cases are still written)
            bad.append("%s: %s: %s" % (name, type(e).__name__, e))
            continue
        if calls != calls2:
            bad.append("%s: the two runs made different calls" % name)
            continue
        cases[name] = {"trace": [table.setdefault(c, len(table)) for c in calls], "sha256": sha if sha == sha2 else None}
        print("%-64s %4d calls  %s" % (name, len(calls), sha[:16] if sha == sha2 else "outputs differ between two runs"), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"calls": [json.loads(c) for c in table], "cases": cases}, f, separators=(",", ":"), sort_keys=True)
    print("%d cases, %d distinct calls, %d bytes -> %s" % (len(cases), len(table), os.path.getsize(args.out), args.out))
    for b in bad:
        print("FAILED " + b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
