"""
Build recipe of the package's native artefacts: libsvmc.so, the closed core (include/svmc.h), libsvmc_ext.so, the first estimator
beside it (include/svmc_ext.h, closed too), and libsvmc_est.so, the open library of estimators beside the core (include/svmc_est.h)
-- hipcc, gfx950 only, in-tree.  It also builds the test-only device probe
tests/native/libsvmc_device_probe.so with the same flags.

    python -m stochvolmodels_amd.build [--force]

hipcc cross-compiles without a GPU; the resulting .so files are git-ignored but travel with the tree.
"""
from __future__ import annotations

import glob
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
INCLUDE = os.path.join(ROOT, "include")
LIB = os.path.join(PKG, "libsvmc.so")
# written beside the library by every build: the instruction histogram of the stepping kernels' time loops, read off the
# compiler's own assembly of THIS build, and the library's sha256 -- bench.py prices its roofline from it and marks the
# line stale when the library it loaded is not the one the histogram describes
ISA_JSON = os.path.join(PKG, "libsvmc.isa.json")
ISA_KERNELS = ("logsv_rng_kernel", "logsv_chain_rng_kernel", "heston_rng_kernelILi0", "heston_rng_kernelILi1", "heston_rng_kernelILi2",
               "logsv_rng_lat_kernelILi4ELi4ELi256", "logsv_chain_rng_lat_kernelILi4ELi4ELi256", "hawkesjd_chain_rng_kernel",
               "logsv_chain_cmc_kernel", "heston_chain_cmc_kernel")
SOURCES = ("svmc_runtime.hip", "svmc_kernels.hip", "svmc_heston.hip", "svmc_rough.hip", "svmc_analytic.hip", "svmc_chain.hip",
           "svmc_comm.hip", "svmc_multi.hip", "svmc_hawkes.hip", "svmc_density.hip", "svmc_cmc.hip", "svmc_greeks.hip")
ASM_GLOB = "*-hip-amdgcn-amd-amdhsa-gfx950.s"       # the device assembly --save-temps leaves, one file per unit
ARCH = "gfx950"
# the test-only device build of the math, complex and Black-76 helpers (tests/test_gpu_device_math.py): not part of the
# package or its C ABI, built here so that it is compiled whenever the library is, with the library's flags
PROBE_SRC = os.path.join(ROOT, "tests", "native", "device_math_probe.hip")
PROBE_LIB = os.path.join(ROOT, "tests", "native", "libsvmc_device_probe.so")
# libsvmc_ext.so (include/svmc_ext.h): the model-agnostic estimators beside the closed core -- one translation unit that links
# nothing from libsvmc.so, built with the library's flags; its kernel metadata goes to a json of its own
EXT_SRC = os.path.join(CSRC, "svmc_ext.hip")
EXT_LIB = os.path.join(PKG, "libsvmc_ext.so")
EXT_ISA_JSON = os.path.join(PKG, "libsvmc_ext.isa.json")
# libsvmc_est.so (include/svmc_est.h): the estimators beside the core, built the way libsvmc_ext.so is.  libsvmc_ext.so is pinned at
# three symbols and four kernels; this one is held to what its header declares, so the next estimator is added to it
EST_SRC = os.path.join(CSRC, "svmc_est.hip")
EST_LIB = os.path.join(PKG, "libsvmc_est.so")
EST_ISA_JSON = os.path.join(PKG, "libsvmc_est.isa.json")


def headers() -> list:
    """every header of csrc/: a header nobody listed cannot leave a stale library behind"""
    return sorted(glob.glob(os.path.join(CSRC, "*.h")))


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC or install ROCm)")


def flags() -> list:
    # --align-all-blocks=4: every basic block starts 16-byte aligned.  The stepping loop's time depends on where its
    # header falls in instruction memory: instruction-for-instruction identical builds measured 3.80 ms (header at
    # +0x6e0) and 4.08 ms (+0x6ec: the 8-byte encodings straddle the fetch granule) on the same box; with aligned
    # blocks every build gets the fast placement (tools/ubench/ab_kernel.py).
    return ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-fno-gpu-rdc",
            "-mllvm", "--align-all-blocks=4", "-I" + INCLUDE, "-I" + CSRC, "-DSVMC_BUILDING=1", "-Wall",
            "-Wno-unused-function", "-Wno-pass-failed"]


def is_stale() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in SOURCES] + headers() + [os.path.join(INCLUDE, "svmc.h"), __file__]
    return any(os.path.getmtime(d) > t for d in deps)


def probe_is_stale() -> bool:
    if not os.path.exists(PROBE_LIB):
        return True
    t = os.path.getmtime(PROBE_LIB)
    deps = [PROBE_SRC, os.path.join(INCLUDE, "svmc.h"), __file__] + headers()
    return any(os.path.getmtime(d) > t for d in deps)


def probe_command() -> list:
    return [hipcc()] + flags() + [PROBE_SRC, "-o", PROBE_LIB]


def build_device_probe(force: bool = False, verbose: bool = False) -> str:
    """tests/native/libsvmc_device_probe.so, rebuilt when its source, a header of csrc/ or svmc.h is newer (about 2 s)"""
    if not os.path.exists(PROBE_SRC) or (not force and not probe_is_stale()):
        return PROBE_LIB
    cmd = probe_command()
    if verbose:
        print(" ".join(cmd))
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if res.returncode != 0:
        raise RuntimeError("hipcc failed on the device probe:\n" + res.stdout + res.stderr)
    if verbose and res.stderr:
        print(res.stderr)
    return PROBE_LIB


def side_is_stale(lib: str, isa_json: str, src: str, header: str) -> bool:
    if not os.path.exists(lib) or not os.path.exists(isa_json):
        return True
    t = os.path.getmtime(lib)
    deps = [src, os.path.join(INCLUDE, "svmc.h"), os.path.join(INCLUDE, header), __file__] + headers()
    return any(os.path.getmtime(d) > t for d in deps)


def build_side(lib: str, isa_json: str, src: str, verbose: bool, extra: tuple = ()) -> str:
    """one translation unit -> a library beside the core; the kernel metadata of the build (kernel_metadata) goes to isa_json in
    libsvmc.isa.json's {"metadata": ...} form"""
    with tempfile.TemporaryDirectory(prefix="svmc_side_build_") as tmp:
        cmd = [hipcc()] + flags() + list(extra) + ["--save-temps", src, "-o", lib]
        if verbose:
            print(" ".join(cmd))
        res = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp)
        if res.returncode != 0:
            raise RuntimeError(f"hipcc failed on {os.path.basename(src)}:\n" + res.stdout + res.stderr)
        if verbose and res.stderr:
            print(res.stderr)
        with open(isa_json, "w") as fh:
            json.dump({"lib_sha256": file_sha256(lib), "flags": flags() + list(extra), "metadata": kernel_metadata(tmp)}, fh, indent=1)
    return lib


def ext_is_stale() -> bool:
    return side_is_stale(EXT_LIB, EXT_ISA_JSON, EXT_SRC, "svmc_ext.h")


def build_ext(force: bool = False, verbose: bool = False) -> str:
    """libsvmc_ext.so, rebuilt when its source, a header of csrc/, either public header or this file is newer; its kernel metadata
    goes to libsvmc_ext.isa.json"""
    if not force and not ext_is_stale():
        return EXT_LIB
    return build_side(EXT_LIB, EXT_ISA_JSON, EXT_SRC, verbose)


def est_is_stale() -> bool:
    return side_is_stale(EST_LIB, EST_ISA_JSON, EST_SRC, "svmc_est.h")


def build_est(force: bool = False, verbose: bool = False) -> str:
    """libsvmc_est.so, rebuilt when its source, a header of csrc/, svmc.h, svmc_est.h or this file is newer; its kernel metadata
    goes to libsvmc_est.isa.json"""
    if not force and not est_is_stale():
        return EST_LIB
    return build_side(EST_LIB, EST_ISA_JSON, EST_SRC, verbose)


def file_sha256(path: str) -> str:
    h = hashlib.sha256()
    with open(path, "rb") as fh:
        for chunk in iter(lambda: fh.read(1 << 20), b""):
            h.update(chunk)
    return h.hexdigest()


def kernel_metadata(asm_dir: str) -> dict:
    """{kernel symbol: {vgpr, sgpr, scratch_bytes, lds_bytes}} of every kernel of this build, read off the amdhsa metadata the
    compiler appends to its assembly -- a spill (scratch_bytes > 0) is visible in the build, not only in a profile"""
    import re
    out = {}
    for path in sorted(glob.glob(os.path.join(asm_dir, ASM_GLOB))):
        text = open(path).read()
        start = text.find("amdhsa.kernels:")
        if start < 0:
            continue
        for block in re.split(r"\n  - ", text[start:])[1:]:
            def field(key, block=block):
                m = re.search(r"\." + key + r":\s*(\S+)", block)
                return m.group(1) if m else None
            name = field("name")
            if name is None:
                continue
            out[name] = {"vgpr": int(field("vgpr_count") or 0), "sgpr": int(field("sgpr_count") or 0),
                         "scratch_bytes": int(field("private_segment_fixed_size") or 0),
                         "lds_bytes": int(field("group_segment_fixed_size") or 0)}
    return out


def write_isa_json(asm_dir: str) -> None:
    """per-kernel instruction histogram of the time loops (tools/isa_histogram.py) + the library's hash; the kernels are looked
    up in the device assembly of every translation unit (asm_dir: where --save-temps left it)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import isa_histogram
    finally:
        sys.path.pop(0)
    text = "\n".join(open(p).read() for p in sorted(glob.glob(os.path.join(asm_dir, ASM_GLOB))))
    kernels = {}
    for name in ISA_KERNELS:
        try:
            kernels[name] = isa_histogram.analyse(text, name)
        except (SystemExit, ValueError) as exc:             # a kernel renamed away: leave it out, bench.py says so
            kernels[name] = {"error": str(exc)}
    with open(ISA_JSON, "w") as fh:
        json.dump({"lib_sha256": file_sha256(LIB), "flags": flags(), "kernels": kernels,
                   "metadata": kernel_metadata(asm_dir)}, fh, indent=1)


def build(force: bool = False, verbose: bool = False) -> str:
    build_device_probe(force, verbose)
    build_ext(force, verbose)
    build_est(force, verbose)
    if not force and not is_stale() and os.path.exists(ISA_JSON):
        return LIB
    # --save-temps: the device assembly of this very compilation is kept for the histogram (temporaries in a scratch dir)
    with tempfile.TemporaryDirectory(prefix="svmc_build_") as tmp:
        cmd = [hipcc()] + flags() + ["--save-temps"] + [os.path.join(CSRC, s) for s in SOURCES] + ["-o", LIB]
        if verbose:
            print(" ".join(cmd))
        res = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp)
        if res.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + res.stdout + res.stderr)
        if verbose and res.stderr:
            print(res.stderr)
        try:
            write_isa_json(tmp)
        except Exception as exc:                             # the histogram is measurement metadata, never a build failure
            if verbose:
                print("isa histogram skipped:", exc)
            if os.path.exists(ISA_JSON):
                os.remove(ISA_JSON)
            with open(ISA_JSON, "w") as fh:
                json.dump({"lib_sha256": file_sha256(LIB), "flags": flags(), "kernels": {}, "error": str(exc)}, fh)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
