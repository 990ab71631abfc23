#!/usr/bin/env python3
"""Does a kernel that gained a trailing compile-time switch (template <..., bool MASKED = false>) still compile to what it was?

    python tools/isa_masked_switch.py <parent csrc dir> <new csrc dir> <file.hip> [<file.hip> ...]

Compiles every file from both directories to gfx950 assembly with the build's flags (bvh_amd/build_ext.py FLAGS without -shared), device
only, with -Rpass-analysis=kernel-resource-usage.  A parent kernel `k<A, B>` is paired with the new `k<A, B, false>` (or with `k<A, B>` where
the kernel gained nothing).  Per pair it prints the remark's figures (TotalSGPRs, VGPRs, AGPRs, scratch, occupancy, LDS) of both sides and
what differs in the instruction text — comments stripped, label numbers masked — as a unified diff; then the figures of every new kernel
that has no parent.  Exit status 0: every paired kernel kept its figures."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bvh_amd.build_ext import FLAGS, hipcc  # noqa: E402

FIGURES = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")
CXXFILT = "c++filt"


def compile_s(src, out):
    """→ {mangled kernel: {figure: value}} from the remarks; the assembly goes to `out`"""
    cmd = [hipcc()] + [f for f in FLAGS if f != "-shared"] + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-o", out, src]
    p = subprocess.run(cmd, cwd=os.path.dirname(src), capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr)
        raise SystemExit(f"hipcc failed on {src}")
    res, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(.+?): (\d+) \[-Rpass-analysis", line)
        if m and cur is not None and m.group(1) in FIGURES:
            cur[m.group(1)] = int(m.group(2))
    return res


def code_of(text, name):
    body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S).group(1)
    desc = re.search(r"^\s*\.amdhsa_kernel\s+%s\n(.*?)\.end_amdhsa_kernel" % re.escape(name), body, re.M | re.S).group(1)
    body = body[:body.index(".amdhsa_kernel")]
    lines = [re.sub(r"\s*;.*$", "", ln).strip() for ln in body.split("\n")]
    code = [re.sub(r"\.LBB\d+_", ".LBB#_", ln) for ln in lines if ln]
    return code, [ln.strip() for ln in desc.split("\n") if ln.strip()]


def demangle(names):
    out = subprocess.run([CXXFILT] + list(names), capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"\(.*$", "", d).replace("void ", "") for n, d in zip(names, out)}


def main():
    parent, new, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for f in files:
            sides = []
            for tag, d in (("parent", parent), ("new", new)):
                out = os.path.join(tmp, f"{tag}_{f}.s")
                res = compile_s(os.path.join(os.path.abspath(d), f), out)
                text = open(out).read()
                kern = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
                names = demangle(kern)
                sides.append((res, text, {names[k]: k for k in kern}))
            (pres, ptext, pk), (nres, ntext, nk) = sides
            print(f"==== {f}: {len(pk)} kernels in the parent, {len(nk)} in this tree")
            paired = set()
            for dn in sorted(pk):
                grown = dn[:-1] + ", false>" if dn.endswith(">") else dn
                twin = grown if grown in nk else dn if dn in nk else None
                if twin is None:
                    print(f"-- {dn}: NO counterpart in this tree")
                    bad += 1
                    continue
                paired.add(twin)
                a, b = pres[pk[dn]], nres[nk[twin]]
                same = a == b
                bad += not same
                print(f"-- {dn}  ->  {twin}")
                print("   parent:    " + ", ".join(f"{k} {a.get(k)}" for k in FIGURES))
                print("   this tree: " + ", ".join(f"{k} {b.get(k)}" for k in FIGURES) + ("   [the same]" if same else "   [DIFFERENT]"))
                (ca, da), (cb, db) = code_of(ptext, pk[dn]), code_of(ntext, nk[twin])
                diff = [ln for ln in difflib.unified_diff(ca, cb, "parent", "this tree", n=0, lineterm="")]
                print(f"   instructions: {len(ca)} lines in the parent, {len(cb)} in this tree, " + ("identical" if not diff else f"{sum(1 for ln in diff if ln[:1] in '+-' and ln[:3] not in ('+++', '---'))} changed lines:"))
                for ln in diff[2:]:
                    print("      " + ln)
                ddiff = [ln for ln in difflib.unified_diff(da, db, "parent", "this tree", n=0, lineterm="") if ln[:1] in "+-" and ln[:3] not in ("+++", "---")]
                print("   kernel descriptor: " + ("identical" if not ddiff else "differs in"))
                for ln in ddiff:
                    print("      " + ln)
            for dn in sorted(set(nk) - paired):
                b = nres[nk[dn]]
                print(f"-- new: {dn}")
                print("   this tree: " + ", ".join(f"{k} {b.get(k)}" for k in FIGURES))
                if b.get("ScratchSize [bytes/lane]") != 0:
                    print("   SCRATCH IN A NEW KERNEL")
                    bad += 1
    print(f"{bad} kernels whose figures moved, lost their counterpart or use scratch")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
