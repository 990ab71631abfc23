#!/usr/bin/env python3
"""Are two sets of device assembly files the same kernels?  python tools/isa_same.py <parent.s ...> -- <new.s ...>
The files come from `hipcc <build_ext.FLAGS without -shared> --cuda-device-only -S`.  Per kernel symbol (whichever file it is in) the
instruction text — comments stripped, the function number in .LBB<n>_ / .Lfunc_end<n> labels masked — and the .amdhsa_kernel block
(registers, LDS, scratch) must be equal, and both sides must hold the same set of kernels.  Exit status 0: the same."""
import re
import sys


def kernels(paths):
    out = {}
    for path in paths:
        text = open(path).read()
        names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
        for name in names:
            body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S).group(1)
            desc = re.search(r"^\s*\.amdhsa_kernel\s+%s\n(.*?)\.end_amdhsa_kernel" % re.escape(name), body, re.M | re.S).group(1)
            body = body[:body.index(".amdhsa_kernel")]   # (the descriptor sits between the code and its end label)
            lines = [re.sub(r"\s*;.*$", "", ln).strip() for ln in body.split("\n")]
            code = re.sub(r"\.LBB\d+_", ".LBB#_", "\n".join(ln for ln in lines if ln))
            assert name not in out, f"{name} is defined twice ({path})"
            out[name] = (code, "\n".join(ln.strip() for ln in desc.split("\n")))
    return out


def main():
    cut = sys.argv.index("--")
    a, b = kernels(sys.argv[1:cut]), kernels(sys.argv[cut + 1:])
    bad = 0
    for name in sorted(set(a) ^ set(b)):
        print(("only in parent: " if name in a else "only in new: ") + name); bad += 1
    for name in sorted(set(a) & set(b)):
        if a[name][0] != b[name][0]:
            print("instructions differ: " + name); bad += 1
        if a[name][1] != b[name][1]:
            print("kernel descriptor differs: " + name); bad += 1
    print(f"{len(a)} kernels in {cut - 1} parent files, {len(b)} kernels in {len(sys.argv) - cut - 1} new files, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
