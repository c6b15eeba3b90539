"""Builds libegonerf_hip.so (gfx950) in-tree with hipcc.  No CPU fallback exists: the product path
raises if this library is missing."""
from __future__ import annotations

import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libegonerf_hip.so")
SOURCES = ["ego_stages.hip", "ego_march.hip", "ego_resample.hip", "ego_runtime.hip", "ego_pack.hip", "ego_shade.hip", "ego_train.hip", "ego_render.hip", "ego_reg.hip", "ego_metrics.hip", "ego_wgrad.hip", "ego_generic.hip", "ego_generic_train.hip", "ego_generic_march.hip", "ego_selftest.hip", "ego_scatter_sorted.hip",
           "ego_scatter_sort.hip", "ego_stage_grad.hip", "ego_compact.hip", "ego_batch.hip", "ego_camera.hip", "ego_msi.hip", "ego_ray_grad.hip", "ego_dense.hip", "ego_geometry.hip", "ego_mesh.hip", "ego_photo.hip", "ego_patch_loss.hip"]
HEADERS = ["ego_device.h", "ego_host.h", "ego_tuned.h", "variants.h", "ego_generic.h", "ego_generic_dev.h", "ego_sorted_geom.h", "ego_vm_grad.h", "ego_march.h", "ego_density.h", os.path.join("..", "..", "include", "egonerf_hip.h")]


def _hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (need ROCm's hipcc to build libegonerf_hip.so)")


TESTED_HIPCC = ("7.2.",)  # HIP versions whose code generation passed the determinism soak of DESIGN.md 5.1


def hipcc_version() -> str:
    out = subprocess.run([_hipcc(), "--version"], capture_output=True, text=True).stdout
    for line in out.splitlines():
        if line.startswith("HIP version:"):
            return line.split(":", 1)[1].strip()
    return "unknown"


def source_hash(extra: list | None = None, per_file: bool = True) -> str:
    """sha256 over the library's sources, headers and compile flags: what `libegonerf_hip.so.hash` records for the binary next
    to it, and what profiles/r*/pmc_traffic.json records for the build its counters were taken from.  `extra` / `per_file`:
    an experiment build's additional flags / dropped per-file flags go into ITS hash, so it can never pass for the product build."""
    import hashlib
    h = hashlib.sha256()
    for f in SOURCES + HEADERS:
        h.update(f.encode())
        h.update(open(os.path.join(CSRC, f), "rb").read())
    h.update(repr((COMMON_FLAGS, sorted(EXTRA_FLAGS.items()))).encode())
    if extra or not per_file:
        h.update(repr((list(extra or []), per_file)).encode())
    return h.hexdigest()[:16]


def stale_reason() -> str | None:
    """None if the binary's recorded source hash equals the tree's (mtimes do not survive a snapshot copy), else why not."""
    if not os.path.exists(LIB):
        return "the library is missing"
    if not os.path.exists(LIB + ".hash"):
        return f"{LIB}.hash is missing (a binary without its recorded source hash cannot be matched to the sources next to it)"
    got = open(LIB + ".hash").read().strip()
    return None if got == source_hash() else f"source hash differs ({got} recorded, {source_hash()} in the tree: other sources, flags, or an experiment build)"


def is_stale() -> bool:
    return stale_reason() is not None


def _code_objects(lib_path: str, workdir: str) -> tuple:
    """The gfx950 code objects inside a built shared library (llvm-objdump --offloading extracts next to its input: work on a copy)."""
    import glob
    objdump = os.path.join(os.path.dirname(os.path.realpath(_hipcc())), "..", "lib", "llvm", "bin", "llvm-objdump")
    if not os.path.exists(objdump):
        objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    copy = os.path.join(workdir, "lib.so")
    shutil.copy(lib_path, copy)
    r = subprocess.run([objdump, "--offloading", copy], capture_output=True, text=True, cwd=workdir)
    if r.returncode != 0:
        raise RuntimeError("llvm-objdump --offloading failed: " + r.stderr[-500:])
    return objdump, sorted(glob.glob(copy + ".*gfx950*"))


def shipped_isa_report(lib_path: str | None = None) -> dict:
    """Disassembles the device code INSIDE the built library (not a fresh compile) and reports the packed fp32 instructions that
    broadcast the high dword of a register pair (`op_sel:[...]` without `op_sel_hi`): the trigger of the fault in DESIGN.md 5.1.
    -> {"code_objects": n, "packed_fp32": n, "high_half_broadcast": [disassembly lines]}"""
    import re
    import tempfile
    lib_path = lib_path or LIB
    with tempfile.TemporaryDirectory() as tmp:
        objdump, cos = _code_objects(lib_path, tmp)
        n_packed, bad = 0, []
        for co in cos:
            dis = subprocess.run([objdump, "-d", co], capture_output=True, text=True).stdout
            for line in dis.splitlines():
                if re.search(r"v_pk_(fma|mul|add)_f32", line):
                    n_packed += 1
                    if "op_sel:" in line and "op_sel_hi" not in line:
                        bad.append(line.strip())
    return dict(code_objects=len(cos), packed_fp32=n_packed, high_half_broadcast=bad)


# Per-source extra flags.  ego_shade.hip is built without the SLP vectoriser: it forms {w00, w01}-style pairs of the interpolation
# weights, and the packed fp32 instructions that then broadcast the high half of such a pair are what every non-reproducible build
# of these kernels had in common.  The source also pins the weights to separate registers; either measure alone
# was enough in every soak, neither costs time.  ego_pack.hip and ego_train.hip were part of ego_shade.hip and keep its flag:
# k_vm_scatter and k_shade_bwd (ego_train.hip) hold the same interpolation-weight arithmetic.
# ego_scatter_sorted.hip (round 5) gets the same flag: with the vectoriser on, k_sorted_plane<16> contained six such instructions,
# and ego_scatter_sort.hip was part of it and keeps its flag (k_sort_keys holds the same coordinate arithmetic);
# so does ego_stage_grad.hip (the stage backward kernels held such instructions with it on), and ego_batch.hip, whose ray
# arithmetic (three dot products per ray) is of the shape the vectoriser pairs up; ego_camera.hip holds the same ray arithmetic, and
# ego_msi.hip dot products of that shape plus bilinear weights applied to four-channel texels; ego_ray_grad.hip holds the
# interpolation-weight arithmetic itself, once more with the weights' derivatives next to them, and ego_geometry.hip the same arithmetic
# again (ego_vm_grad.h), as does ego_mesh.hip (the point gradients, and the lattice field's density_lookup); ego_photo.hip holds
# per-channel multiply-add triples (gain * rgb + bias over three channels) of the shape the vectoriser pairs, and ego_patch_loss.hip the five
# window moments and the three coefficient fields of the structural term: tap-weighted sums taken side by side, the same shape.
EXTRA_FLAGS = {"ego_shade.hip": ["-fno-slp-vectorize"], "ego_pack.hip": ["-fno-slp-vectorize"], "ego_train.hip": ["-fno-slp-vectorize"],
               "ego_scatter_sorted.hip": ["-fno-slp-vectorize"], "ego_scatter_sort.hip": ["-fno-slp-vectorize"],
               "ego_stage_grad.hip": ["-fno-slp-vectorize"], "ego_batch.hip": ["-fno-slp-vectorize"],
               "ego_camera.hip": ["-fno-slp-vectorize"], "ego_msi.hip": ["-fno-slp-vectorize"],
               "ego_ray_grad.hip": ["-fno-slp-vectorize"], "ego_geometry.hip": ["-fno-slp-vectorize"],
               "ego_mesh.hip": ["-fno-slp-vectorize"], "ego_photo.hip": ["-fno-slp-vectorize"],
               "ego_patch_loss.hip": ["-fno-slp-vectorize"]}
COMMON_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-munsafe-fp-atomics", "-fPIC"]


def build_library(force: bool = False, verbose: bool = False, extra: list | None = None, out: str | None = None) -> str:
    """`extra` (or the environment variable EGO_EXTRA_FLAGS) adds compiler flags to every source and `out` names another output
    file: experiment builds (tools/variant_test.sh)."""
    extra = list(extra or []) + os.environ.get("EGO_EXTRA_FLAGS", "").split()
    out = out or os.environ.get("EGO_LIB_OUT") or LIB
    if not force and not extra and out == LIB and not is_stale():
        return LIB
    ver = hipcc_version()
    if not ver.startswith(TESTED_HIPCC) and not os.environ.get("EGO_ALLOW_UNTESTED_HIPCC"):
        # a code-generation-dependent fault was found and fenced off with this compiler; another one must
        # pass tests/test_hip_determinism.py (3000 repetitions per op) before its binaries are trusted
        raise RuntimeError(f"hipcc {ver} is not a tested compiler ({TESTED_HIPCC}); set EGO_ALLOW_UNTESTED_HIPCC=1 to build anyway "
                           "and run tests/test_hip_determinism.py on the result")
    objdir = os.path.join(HERE, "build" + ("_" + os.path.basename(out) if out != LIB else ""))
    os.makedirs(objdir, exist_ok=True)
    procs, objs = [], []
    for f in SOURCES:  # one hipcc per source, in parallel: the sources have no device-side references to one another
        obj = os.path.join(objdir, f.replace(".hip", ".o"))
        objs.append(obj)
        per_file = [] if os.environ.get("EGO_NO_PER_FILE_FLAGS") else EXTRA_FLAGS.get(f, [])  # experiments only
        cmd = [_hipcc(), *COMMON_FLAGS, *per_file, *extra, "-c", os.path.join(CSRC, f), "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((f, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for f, pr in procs:
        log, _ = pr.communicate()
        if pr.returncode != 0:
            raise RuntimeError(f"hipcc failed on {f}:\n" + log)
    cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", out + ".tmp"]
    if verbose:
        print(" ".join(cmd))
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc (link) failed:\n" + r.stdout + r.stderr)
    os.replace(out + ".tmp", out)
    # every build records ITS hash next to the binary: an experiment build written over LIB (extra flags / no per-file flags) gets a
    # hash that differs from the tree's, so _lib.load() refuses it unless EGO_ALLOW_STALE_LIB=1 (it used to keep the old .hash)
    open(out + ".hash", "w").write(source_hash(extra, per_file=not os.environ.get("EGO_NO_PER_FILE_FLAGS")) + "\n")
    if out != LIB:
        shutil.rmtree(objdir, ignore_errors=True)
    return out


if __name__ == "__main__":
    print(build_library(force=True, verbose=True))
