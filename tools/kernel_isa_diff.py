#!/usr/bin/env python3
"""Kernel-by-kernel diff of the gfx950 assembly of this tree against a parent commit.

  python tools/kernel_isa_diff.py [--rev REV] [-D NAME ...] [FILE.hip ...]
  (REV defaults to HEAD; -D: the parent's defines; files default to all of HIP_SOURCES)

Every file of build.py's HIP_SOURCES is compiled twice with `--cuda-device-only -S` and build.py's flags
for that file: REV's csrc/ with the given -D switches, this tree's with DEFAULT_DEFINES.  Functions are
compared by their instruction text (comments, .loc/.file lines and the function index inside local
labels normalised away) and by their kernel-descriptor values.  It only diffs; it looks for no
instruction."""
import argparse, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from compliancedex_amd import build as B

DESC = ("next_free_vgpr", "accum_offset", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")


def asm(root, src, defines, out):
    flags = ["-O3", "-std=c++17", f"--offload-arch={B.ARCH}", "-Wno-pass-failed", "-I", os.path.join(root, "include")]
    flags += [f"-D{d}" for d in defines]
    flags += ["-ffp-contract=off"] if src in B.FP_CONTRACT_OFF else []
    subprocess.run([B.HIPCC, *flags, "--cuda-device-only", "-S", os.path.join(root, "compliancedex_amd", "csrc", src),
                    "-o", out], check=True)
    return parse(open(out).read())


def parse(text):
    """{function: (normalised instruction lines, {descriptor field: value})}"""
    fns = {}
    for m in re.finditer(r"^\s*\.type\s+(\S+),@function\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        body = m.group(2).split("\n\t.section")[0]  # (the kernel descriptor follows in .rodata)
        lines = [re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0]).strip() for l in body.splitlines()]
        fns[m.group(1)] = ([l for l in lines if l and not l.startswith((".loc", ".file", ".cfi", ".p2align"))], {})
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)\.end_amdhsa_kernel", text, re.M | re.S):
        fns[m.group(1)][1].update((k, v) for k, v in re.findall(r"\.amdhsa_(\w+)\s+(\S+)", m.group(2)) if k in DESC)
    return fns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rev", default="HEAD")
    ap.add_argument("-D", dest="pdef", action="append", default=[])
    ap.add_argument("files", nargs="*", default=B.HIP_SOURCES)
    a = ap.parse_args()
    rev, pdef, srcs = a.rev, a.pdef, a.files
    removed, same, differ = [], [], []
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", B.REPO, "archive", rev, "compliancedex_amd/csrc", "include"],
                             check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        jobs = [(r, s, d, os.path.join(tmp, f"{t}.{s}.s")) for s in srcs
                for r, d, t in ((tmp, pdef, "old"), (B.REPO, B.DEFAULT_DEFINES, "new"))]
        with ThreadPoolExecutor(int(os.environ.get("CDX_BUILD_JOBS", "4"))) as ex:
            res = list(ex.map(lambda j: asm(*j), jobs))
    for src, old, new in zip(srcs, res[0::2], res[1::2]):
        for k in sorted(set(old) | set(new)):
            name = f"{src}: {k}"
            if k not in new:
                removed.append(name)
            elif k not in old:
                differ.append(name + "  (new function)")
            elif old[k] == new[k]:
                same.append(name)
            else:
                (ot, od), (nt, nd) = old[k], new[k]
                n = lambda t: sum(not l.endswith(":") for l in t)  # (labels are not instructions)
                what = ["text identical" if ot == nt else f"instructions {n(ot)} -> {n(nt)}"]
                what += [f"{f} {od.get(f)}" + (f" -> {nd.get(f)}" if od.get(f) != nd.get(f) else "")
                         for f in DESC if ot != nt or od.get(f) != nd.get(f)]
                differ.append(name + "  (" + "; ".join(what) + ")")
    for title, rows in (("removed", removed), ("identical", same), ("differ", differ)):
        print(f"== {title}: {len(rows)}")
        print("".join(f"  {r}\n" for r in rows), end="")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
