#!/usr/bin/env python3
"""Per-kernel comparison of two source trees' gfx950 code, without a GPU: every file is compiled to assembly with the
Makefile's flags (hipcc --cuda-device-only -S) in both trees; per kernel the registers, LDS and scratch bytes of the
code-object metadata, the waves per SIMD they allow, and whether the instruction sequences (comments, labels' directives and
blank lines dropped) are equal.  Kernels are matched by their demangled name without the parameter list, so a kernel that gained a
parameter is still compared with its parent; a kernel (an instantiation) that only the new tree has is listed by itself like
the kernels of a new file (`new_kernel`).  A file that only the new tree has is listed by itself (`new_file`, no parent figures): its
kernels are within the rules when they use no scratch.

  python profiles/code_object_diff.py <parent csrc dir> <new csrc dir> out.json k5_window.hip k13_texture.hip ..."""
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def makefile_flags(csrc):
    """CXXFLAGS of the tree's own Makefile ($(ARCH) filled in from its ARCH line), so the comparison follows the build."""
    text = open(os.path.join(csrc, "Makefile")).read()
    arch = re.search(r"^ARCH \?= *(\S+)", text, re.M).group(1)
    return re.search(r"^CXXFLAGS \?= *(.*)$", text, re.M).group(1).replace("$(ARCH)", arch).split()


def asm(csrc, f, tmp, tag):
    out = os.path.join(tmp, f"{tag}_{f}.s")
    subprocess.check_call([HIPCC, *makefile_flags(csrc), "--cuda-device-only", "-S", f, "-o", out], cwd=csrc, stderr=subprocess.DEVNULL)
    return open(out).read()


def demangle(names):
    p = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, p.stdout.split("\n")))


def short(demangled):
    return demangled.split("(")[0].replace("void ", "")


def by_name(kn):
    """mangled -> figures becomes demangled name without parameters -> figures; kernels that share that name (overloads, as in
    k16_forest_fit.hip) keep their parameter list"""
    names = demangle(sorted(kn))
    count = {}
    for m in kn:
        count[short(names[m])] = count.get(short(names[m]), 0) + 1
    out = {(short(names[m]) if count[short(names[m])] == 1 else names[m].replace("void ", "")): v for m, v in kn.items()}
    assert len(out) == len(kn), "two kernels share a name"
    return out


def kernels(text):
    res = {}
    for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M):
        # a local label carries the number of its function in the file (.LBB12_3), which moves when a kernel is added before it
        ins = [re.sub(r"\.L(\w+?)\d+_(\d+)", r".L\1_\2", ln.split(";")[0].strip()) for ln in m.group(2).split("\n")]
        res[m.group(1)] = {"ins": [i for i in ins if i and not i.startswith(".")]}
    for m in re.finditer(r"- \.agpr_count:.*?\.name:\s+(\w+).*?\.wavefront_size", text, re.S):
        blk, name = m.group(0), m.group(1)
        if name in res:
            for key, field in (("vgprs", "vgpr_count"), ("agprs", "agpr_count"), ("sgprs", "sgpr_count"), ("lds", "group_segment_fixed_size"),
                               ("scratch", "private_segment_fixed_size"), ("wg", "max_flat_workgroup_size")):
                res[name][key] = int(re.search(r"\." + field + r":\s+(\d+)", blk).group(1))
    return res


def waves_per_simd(k):
    """gfx950: 512 registers per SIMD lane shared by VGPRs and AGPRs in granules of 8, at most 8 waves per SIMD; 160 KB of LDS
    per CU shared by the workgroups of its 4 SIMDs.  (The SGPR limit and the LDS allocation granule are ignored: neither binds
    below 100 SGPRs and with tiles of 9-42 KB.)"""
    regs = -(-k["vgprs"] // 8) * 8 + -(-k["agprs"] // 8) * 8
    w = min(8, 512 // max(regs, 8))
    if k["lds"]:
        w = min(w, (160 * 1024 // k["lds"]) * -(-k["wg"] // 64) // 4)
    return w


def main():
    parent, new, outp, files = sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4:]
    table = []
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(8) as ex:
        jobs = {(t, f): ex.submit(asm, c, f, tmp, t) for f in files for t, c in (("parent", parent), ("new", new))
                if os.path.exists(os.path.join(c, f))}
        for f in files:
            if ("parent", f) not in jobs:      # a file the parent does not have: its kernels alone, the rule is no scratch
                kn = kernels(jobs[("new", f)].result())
                names = demangle(sorted(kn))
                for name in sorted(kn):
                    b = kn[name]
                    row = {"file": f, "kernel": names[name].split("(")[0].replace("void ", ""), "new_file": True}
                    for k in ("vgprs", "sgprs", "lds", "scratch"):
                        row[k] = [None, b[k]]
                    row["waves_per_simd"] = [None, waves_per_simd(b)]
                    row["instructions"] = [None, len(b["ins"])]
                    row["identical"] = None
                    row["within_the_rules"] = b["scratch"] == 0
                    table.append(row)
                    print("new  " + ("" if row["within_the_rules"] else "RULE ") + json.dumps(row))
                continue
            kp, kn = by_name(kernels(jobs[("parent", f)].result())), by_name(kernels(jobs[("new", f)].result()))
            assert set(kp) <= set(kn), (f, set(kp) - set(kn))
            for name in sorted(set(kn) - set(kp)):      # an instantiation the parent does not have: the rule is no scratch
                b = kn[name]
                row = {"file": f, "kernel": name, "new_kernel": True}
                for k in ("vgprs", "agprs", "sgprs", "lds", "scratch"):
                    row[k] = [None, b[k]]
                row["waves_per_simd"] = [None, waves_per_simd(b)]
                row["instructions"] = [None, len(b["ins"])]
                row["identical"] = None
                row["within_the_rules"] = b["scratch"] == 0
                table.append(row)
                print("new  " + ("" if row["within_the_rules"] else "RULE ") + json.dumps(row))
            for name in sorted(kp):
                a, b = kp[name], kn[name]
                row = {"file": f, "kernel": name}
                for k in ("vgprs", "agprs", "sgprs", "lds", "scratch"):
                    row[k] = [a[k], b[k]]
                row["waves_per_simd"] = [waves_per_simd(a), waves_per_simd(b)]
                row["instructions"] = [len(a["ins"]), len(b["ins"])]
                row["identical"] = a["ins"] == b["ins"]
                row["within_the_rules"] = b["scratch"] == 0 and a["lds"] == b["lds"] and row["waves_per_simd"][1] >= row["waves_per_simd"][0]
                table.append(row)
                print(("same " if row["identical"] else "DIFF ") + ("" if row["within_the_rules"] else "RULE ") + json.dumps(row))
    json.dump(table, open(outp, "w"), indent=1)


main()
