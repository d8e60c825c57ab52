#!/usr/bin/env python3
"""Device assembly of two source trees of this project, side by side: every unit of build.UNITS compiled with
build.HIPCC_FLAGS (+ extra flags) --cuda-device-only -S, the per-file __hip_cuid_* lines dropped, split at the kernel
symbols; per kernel "same" or the number of differing lines, plus the two resource rows where they differ.  The compiler numbers
its local labels by the function's position in the unit (.LBB3_7, .Lfunc_end3, "Header=BB3_4"): that index is blanked, and the
.section / .globl lines that open a function count with it, not with the one before -- a function added to a unit does not
make its neighbours differ.
   python tools/asm_diff.py [--units pcc_small,pcc_retire] [--keep DIR] [--jobs N] TREE_A TREE_B [-- -DPCC_PROFILE=1 ...]
The first line of the report names the two trees as given and the flags."""
import argparse, difflib, importlib.util, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor


def load_build(tree):
    spec = importlib.util.spec_from_file_location("build_" + str(abs(hash(tree))), os.path.join(tree, "pcc-rl_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def resource_rows(remarks):
    """{kernel symbol: {field: value}} from the compiler's -Rpass-analysis=kernel-resource-usage remarks."""
    rows, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark: (?:\S+:\d+:\d+: )?\s*(.+?):\s*(\S+)\s+\[-Rpass-analysis", line)
        if m and m.group(1) == "Function Name":
            cur = rows.setdefault(m.group(2), {})
        elif m and cur is not None:
            cur[m.group(1)] = m.group(2)
    return rows


def compile_unit(build, unit, extra, out):
    """-> ({symbol: [lines]}, {kernel: resource row}) of one unit; chunk "" is what precedes the first function."""
    cmd = ["hipcc"] + build.HIPCC_FLAGS + list(extra) + ["-I", build.INCLUDE, "-I", build.CSRC, "-Rpass-analysis=kernel-resource-usage",
                                                        "--cuda-device-only", "-S", os.path.join(build.CSRC, unit), "-o", out]
    p = subprocess.run(cmd, stderr=subprocess.PIPE, universal_newlines=True)
    if p.returncode != 0:
        raise RuntimeError("%s failed:\n%s" % (" ".join(cmd), p.stderr[-4000:]))
    chunks, cur, opening = {"": []}, "", []
    with open(out) as f:
        for line in f:
            if "__hip_cuid" in line:
                continue
            line = re.sub(r"(BB|\.Lfunc_begin|\.Lfunc_end|\.Ltmp)\d+", r"\1#", line)
            if re.match(r"\s*\.(section\s+\.text|globl|protected|weak|hidden|p2align)\b", line):
                opening.append(line)   # (of the function whose .type line follows)
                continue
            m = re.match(r"\s*\.type\s+(\S+),@function", line)
            if m:
                cur = m.group(1)
                chunks[cur] = opening
                opening = []
            else:
                if line.startswith("\t.amdgpu_metadata") or line.startswith("\t.section\t.AMDGPU.gpr_maximums") or re.match(r"\s*\.type\s+\S+,@object", line):
                    cur = ""   # (descriptors and metadata: symbol names, kernarg layouts, register counts)
                if opening:    # (they opened no function: they stay with what they stand in -- an object's go outside with it)
                    chunks[cur] += opening
                    opening = []
            chunks[cur].append(line)
    return chunks, resource_rows(p.stderr)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--units", default="", help="comma-separated unit names (default: build.UNITS of tree B)")
    ap.add_argument("--keep", default=None, help="keep the .s files here (a/ and b/)")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    argv = sys.argv[1:]   # (everything after a "--" goes to the compiler, wherever the options stand)
    cut = argv.index("--") if "--" in argv else len(argv)
    a = ap.parse_args(argv[:cut])
    a.flags = argv[cut + 1:]
    builds = [load_build(os.path.abspath(a.tree_a)), load_build(os.path.abspath(a.tree_b))]
    units = [u if u.endswith(".hip") else u + ".hip" for u in a.units.split(",") if u] or builds[1].UNITS
    keep = a.keep or tempfile.mkdtemp(prefix="asm_diff_")
    for side in "ab":
        os.makedirs(os.path.join(keep, side), exist_ok=True)
    with ThreadPoolExecutor(a.jobs) as ex:
        jobs = {(u, k): ex.submit(compile_unit, builds[k], u, a.flags, os.path.join(keep, "ab"[k], u[:-4] + ".s")) for u in units for k in (0, 1)}
        res = {key: j.result() for key, j in jobs.items()}
    print("# %s vs %s, flags: %s" % (a.tree_a, a.tree_b, " ".join(builds[1].HIPCC_FLAGS + a.flags)))
    differing = 0
    for u in units:
        (ca, ra), (cb, rb) = res[(u, 0)], res[(u, 1)]
        rows = []
        for sym in sorted(set(ca) | set(cb)):
            la, lb = ca.get(sym), cb.get(sym)
            if la == lb:
                continue
            name = sym or "(outside functions: descriptors, metadata)"
            if la is None or lb is None:
                rows.append("  %s: only in %s" % (name, "B" if la is None else "A"))
            else:
                n = sum(1 for d in difflib.unified_diff(la, lb, n=0, lineterm="") if d[:1] in "+-" and d[:3] not in ("+++", "---"))
                rows.append("  %s: %d differing lines of %d / %d" % (name, n, len(la), len(lb)))
            if ra.get(sym) != rb.get(sym):
                rows.append("    A: %s\n    B: %s" % (ra.get(sym), rb.get(sym)))
        n_dev = sum(1 for s in cb if s)
        print("%s: %s" % (u, "same (%d functions, %d lines)" % (n_dev, sum(map(len, cb.values()))) if not rows else "DIFFERENT"))
        for r in rows:
            print(r)
        differing += bool(rows)
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
