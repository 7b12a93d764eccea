"""Build libitsd_hip.so in-tree: hipcc --offload-arch=gfx950, one object per .hip,
linked into a shared library next to this file (travels to the GPU box with the
repo snapshot; no JIT cache involved)."""
from __future__ import annotations

import concurrent.futures as cf
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(HERE), "include")
OBJ = os.path.join(HERE, "build")
LIB = os.path.join(HERE, "libitsd_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"
FLAGS = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-I", CSRC, "-I", INCLUDE,
         "-Wno-unused-result", "-munsafe-fp-atomics"]
# conv.hip: no SLP packing of scalar f32 into v_pk_* -- packed f32 VALU issued beside MFMAs
# (the fused GroupNorm conv's halo transform) costs ~22 cycles an instruction on gfx950
# (MI355X_MICROARCH.md, 'price of one filler'); measured: halo staging 14.1k -> 10.1k cycles
# per 64-channel chunk (profiles/r02_ws_phase_stamps_scalar.txt)
FILE_FLAGS = {"conv.hip": ["-fno-slp-vectorize"]}


def sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))


def _needs(obj, deps):
    if not os.path.exists(obj):
        return True
    t = os.path.getmtime(obj)
    return any(os.path.getmtime(d) > t for d in deps)


def flags_for(src, defines=()):
    """The compile flags of one .hip file (the diagnostic builds and tools/regs.py use the same)."""
    return FLAGS + FILE_FLAGS.get(os.path.basename(src), []) + list(defines)


def build(verbose: bool = False, force: bool = False, defines=(), obj_dir: str = OBJ, lib: str = LIB) -> str:
    """defines / obj_dir / lib: a variant library (extra hipcc definitions, its own objects, its own output)."""
    os.makedirs(obj_dir, exist_ok=True)
    # every file a .hip may include (headers and .inc fragments) is a dependency of every object
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".inc"))]
    headers.append(os.path.join(INCLUDE, "itsd.h"))
    jobs = []
    objs = []
    for src in sources():
        obj = os.path.join(obj_dir, os.path.basename(src)[:-4] + ".o")
        objs.append(obj)
        if force or _needs(obj, [src] + headers):
            jobs.append([HIPCC] + flags_for(src, defines) + ["-c", src, "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed:\n{' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
        return r

    with cf.ThreadPoolExecutor(max_workers=min(8, max(1, len(jobs)))) as ex:
        list(ex.map(run, jobs))
    if force or jobs or _needs(lib, objs):
        run([HIPCC, "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", lib] + objs)
    return lib


if __name__ == "__main__":
    # python build.py [--force] [--obj-dir DIR] [--out LIB] [-DNAME[=VALUE] ...]
    argv = sys.argv[1:]
    opt = {"--obj-dir": OBJ, "--out": LIB}
    for k in opt:
        if k in argv:
            opt[k] = os.path.abspath(argv[argv.index(k) + 1])
    print(build(verbose=True, force="--force" in argv, defines=[a for a in argv if a.startswith("-D")],
                obj_dir=opt["--obj-dir"], lib=opt["--out"]))
