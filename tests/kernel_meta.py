"""Code-object metadata of the kernels of one csrc translation unit, for the CPU tests that hold register / scratch / LDS
budgets.  The source is compiled the way tools/kernel_resources.sh does (hipcc --offload-arch=gfx950 -O3 --save-temps) and
the numbers are read from the amdhsa.kernels records in the device assembly.  A source is compiled once per process:
several test modules ask for csrc/edge.hip."""
import os
import re
import shutil
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "yolat_vectorgraphicsrecognition_amd", "csrc")
KEYS = (".vgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size",
        ".max_flat_workgroup_size")
_DONE = {}


def find_hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.isfile(cand) and os.access(cand, os.X_OK):
            return cand
    return None


def kernel_resources(src):
    """{mangled kernel name: {metadata key: int}} of every kernel of one translation unit"""
    src = os.path.abspath(src)
    if src in _DONE:
        return _DONE[src]
    base = os.path.splitext(os.path.basename(src))[0]
    with tempfile.TemporaryDirectory(prefix="kres_") as workdir:
        r = subprocess.run([find_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--save-temps", "-o",
                            os.path.join(workdir, base + ".o"), src], cwd=workdir, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-4000:]
        asm = os.path.join(workdir, base + "-hip-amdgcn-amd-amdhsa-gfx950.s")
        assert os.path.isfile(asm), os.listdir(workdir)
        with open(asm) as f:
            text = f.read()
    out = {}
    # the amdhsa.kernels metadata: one "- .agpr_count: ..." record per kernel, keys in alphabetical order
    for rec in text[text.index("amdhsa.kernels:"):].split("\n  - ")[1:]:
        name = re.search(r"^    \.name:\s+(\S+)", rec, re.M)       # (4 spaces: the kernel's, not an argument's)
        if not name:
            continue
        cur = {}
        for k in KEYS:
            m = re.search(r"^    %s:\s+(\d+)" % re.escape(k), rec, re.M)
            assert m, (name.group(1), k)
            cur[k] = int(m.group(1))
        out[name.group(1)] = cur
    _DONE[src] = out
    return out


def one(resources, prefix):
    hits = [k for k in resources if k.startswith(prefix)]
    assert len(hits) == 1, (prefix, hits)
    print(hits[0][:60], resources[hits[0]])
    return resources[hits[0]]
