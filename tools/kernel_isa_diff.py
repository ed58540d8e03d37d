#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the gfx950 device assembly of two csrc trees.

    python tools/kernel_isa_diff.py [--per-file] <csrc_a> <csrc_b>

Every .hip of both trees is compiled the way tools/kernel_resources.sh does (hipcc --offload-arch=gfx950 -O3 -std=c++17
--save-temps, at most 16 at a time).  The device assembly is cut into one text per function symbol — the body from its
label to its end label, and for a kernel its .amdhsa_kernel descriptor — with comments stripped and the per-function
index of the block labels (.LBB<n>_) normalised, since that index only counts the functions in front of it in the file.
One line per symbol: SAME, DIFF, ONLY-A or ONLY-B; the SAME kernels of a library namespace (rocprim's sort kernels,
several hundred long names) are compared like the rest and counted on one line.  A symbol that several translation
units emit (the static kernels of gemm_tn.hpp, template instances of a shared header) is SAME only when the two trees
give it the same SET of texts: the compiler does not always give one source the same instructions in every translation
unit (k_gemm_nt_two had two forms within one tree while every file included it), so a kernel that moves into a new file can come out
changed, and that is a DIFF.  The exit status is 0 only when every line is SAME: a change that only moves kernels
between files passes, anything that changes what a kernel executes or the resources it declares does not.

--per-file compares the .hip files of the two trees by name instead, symbol by symbol: SAME or DIFF where both files emit
the symbol, GONE for a symbol that only the old file emits, NEW for one that only the new file emits (a file that exists
in one tree only counts as empty in the other).  The exit status is 0 when there is no DIFF and no NEW.  This is the
mode for a change that takes dead copies of a kernel out of translation units that never launch it: in the whole-tree
mode the symbol's set of texts shrinks, which is a DIFF there."""
import concurrent.futures
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile


def find_hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.isfile(cand) and os.access(cand, os.X_OK):
            return cand
    sys.exit("kernel_isa_diff: no hipcc")


def device_asm(hipcc, src, workdir):
    base = os.path.splitext(os.path.basename(src))[0]
    os.makedirs(workdir)
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--save-temps", "-o",
                        os.path.join(workdir, base + ".o"), src], cwd=workdir, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("kernel_isa_diff: %s does not compile\n%s" % (src, r.stderr[-4000:]))
    with open(os.path.join(workdir, base + "-hip-amdgcn-amd-amdhsa-gfx950.s")) as f:
        return f.read()


def clean(lines):
    out = []
    for ln in lines:
        ln = re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0]).strip()
        if ln:
            out.append(ln)
    return "\n".join(out)


def functions(asm):
    """{symbol: normalised text} of every function of one device assembly file"""
    lines = asm.split("\n")
    syms = {m.group(1) for m in (re.match(r"\s*\.type\s+(\S+),@function", ln) for ln in lines) if m}
    out, cur, start = {}, None, 0
    for i, ln in enumerate(lines):
        if cur is None:
            m = re.match(r"(\S+):", ln) or re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
            if m and m.group(1) in syms:
                cur, start = m.group(1), i + (ln[0] not in " \t")        # (the label itself is dropped, the directive kept)
        elif ln.startswith(".Lfunc_end") or ln.strip() == ".end_amdhsa_kernel":
            out[cur] = out.get(cur, "") + clean(lines[start:i]) + "\n"
            cur = None
    assert cur is None and set(out) == syms, sorted(syms - set(out))
    return out


def tree(hipcc, csrc, workdir, pool):
    """{file name: {symbol: text}} of the tree's translation units"""
    srcs = sorted(glob.glob(os.path.join(csrc, "*.hip")))
    if not srcs:
        sys.exit("kernel_isa_diff: no .hip under %s" % csrc)
    jobs = [pool.submit(device_asm, hipcc, os.path.abspath(s), os.path.join(workdir, os.path.basename(s))) for s in srcs]
    return {os.path.basename(s): functions(j.result()) for s, j in zip(srcs, jobs)}


def texts(files):
    """{symbol: set of the texts the tree's translation units give it}"""
    out = {}
    for syms in files.values():
        for sym, text in syms.items():
            out.setdefault(sym, set()).add(text)
    return out


def library_name(sym):
    """the named namespace of a symbol that is not the anonymous one (library code: rocprim), else None"""
    ns = re.match(r"_ZN(\d+)", sym)
    if ns and not sym.startswith("_ZN12_GLOBAL__N_1"):
        return sym[3 + len(ns.group(1)):][:int(ns.group(1))]
    return None


def per_file(a, b):
    bad, total, lib_same = 0, 0, {}
    for name in sorted(set(a) | set(b)):
        fa, fb = a.get(name, {}), b.get(name, {})
        for sym in sorted(set(fa) | set(fb)):
            if sym not in fb:
                verdict = "GONE"
            elif sym not in fa:
                verdict = "NEW"
            else:
                verdict = "SAME" if fa[sym] == fb[sym] else "DIFF"
            total += 1
            bad += verdict in ("DIFF", "NEW")
            lib = library_name(sym)
            if verdict == "SAME" and lib:
                lib_same[lib] = lib_same.get(lib, 0) + 1
            else:
                print("%-4s %-16s %s" % (verdict, name, sym))
    for lib, n in sorted(lib_same.items()):
        print("SAME %s:: %d kernels" % (lib, n))
    print("%d symbols in %d files, %d DIFF or NEW" % (total, len(set(a) | set(b)), bad))
    return 1 if bad else 0


def main():
    args = [x for x in sys.argv[1:] if x != "--per-file"]
    if len(args) != 2:
        sys.exit(__doc__)
    hipcc = find_hipcc()
    with tempfile.TemporaryDirectory(prefix="isa_diff_") as work, concurrent.futures.ThreadPoolExecutor(16) as pool:
        a = tree(hipcc, args[0], os.path.join(work, "a"), pool)
        b = tree(hipcc, args[1], os.path.join(work, "b"), pool)
    if len(args) < len(sys.argv) - 1:
        return per_file(a, b)
    a, b = texts(a), texts(b)
    bad, lib_same = 0, {}
    for sym in sorted(set(a) | set(b)):
        if sym not in b:
            verdict = "ONLY-A"
        elif sym not in a:
            verdict = "ONLY-B"
        else:
            verdict = "SAME" if a[sym] == b[sym] else "DIFF"
        bad += verdict != "SAME"
        name = library_name(sym)
        if verdict == "SAME" and name:
            lib_same[name] = lib_same.get(name, 0) + 1
        else:
            print("%-6s %s" % (verdict, sym))
    for name, n in sorted(lib_same.items()):
        print("SAME   %s:: %d kernels" % (name, n))
    print("%d symbols, %d not SAME" % (len(set(a) | set(b)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
