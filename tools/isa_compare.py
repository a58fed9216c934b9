#!/usr/bin/env python3
"""Compare the device assembly of one source at two commits, kernel by kernel.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 [-mllvm -amdgpu-mfma-vgpr-form] --offload-device-only -S x.hip -o x.s

    tools/isa_compare.py before.s after.s [--rename OLD=NEW]... [--markdown]

Per kernel symbol: VGPRs, SGPRs, scratch bytes, static LDS bytes (the code object's metadata) and the number of
instructions in its body.  Exit status 1 when the sets of symbols differ or any figure does.  --rename maps a substring of
the old mangled names (an argument struct that was renamed) before the comparison; it may be given more than once."""
import re
import sys

FIELDS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def kernels(path):
    text = open(path).read()
    out = {}
    for entry in re.split(r"^  - ", text[text.rfind("amdhsa.kernels:"):], flags=re.M)[1:]:   # keys sorted; one entry per kernel
        f = dict(re.findall(r"^\s+(\.[a-z_]+):\s+(\S+)$", "    " + entry, re.M))
        if ".name" not in f:                              # (the version list behind the kernels)
            continue
        name = f[".name"]
        body = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end" % re.escape(name), text, re.S | re.M).group(1)
        n_instr = sum(1 for ln in body.splitlines() if re.match(r"\s+[a-z]", ln))
        out[name] = tuple(int(f[k]) for k in FIELDS) + (n_instr,)
    return out


def main(argv):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--rename", metavar="OLD=NEW", action="append", default=[])
    ap.add_argument("--markdown", action="store_true")
    ns = ap.parse_args(argv)
    before, after = kernels(ns.before), kernels(ns.after)
    for ren in ns.rename:
        old, new = ren.split("=", 1)
        before = {k.replace(old, new): v for k, v in before.items()}
    bad = sorted(set(before) ^ set(after))
    for k in bad:
        print("only in %s: %s" % ("before" if k in before else "after", k))
    md = ns.markdown
    if md:
        print("| kernel | VGPRs | SGPRs | scratch B | static LDS B | instructions |")
        print("|---|---|---|---|---|---|")
    ndiff = 0
    for k in sorted(set(before) & set(after)):
        b, a = before[k], after[k]
        ndiff += b != a
        cell = ["%d" % x if x == y else "**%d -> %d**" % (x, y) for x, y in zip(b, a)]
        if md:
            print("| `%s` | %s |" % (k, " | ".join(cell)))
        elif b != a:
            print("DIFF %s: %s" % (k, " ".join(cell)))
    print("\n%d kernels, %d with a different figure, %d unmatched" % (len(set(before) & set(after)), ndiff, len(bad)))
    return 1 if bad or ndiff else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
