"""Builds libdistdiff_hip.so (hand-written gfx950 kernels + engine + C ABI) and its fp16 variant libdistdiff_hip_f16.so in-tree with hipcc.

    python -m distdiff_amd.build            # incremental
    python -m distdiff_amd.build --force

hipcc cross-compiles for gfx950 without a GPU; the .so is git-ignored but travels with gpurun.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
# DD_BUILD_OBJ / DD_BUILD_LIB: a variant build beside the product one (A/B of compile-time switches: DD_EXTRA_CFLAGS=-D... ; run with DD_LIB=)
OBJ = os.environ.get("DD_BUILD_OBJ") or os.path.join(HERE, "csrc", "_obj")
LIB = os.environ.get("DD_BUILD_LIB") or os.path.join(HERE, "libdistdiff_hip.so")
SOURCES = ["conv_gemm.hip", "conv_gemm2.hip", "conv_halo.hip", "gemm_pps.hip", "gemm_ws.hip", "norm.hip", "attention.hip", "attention_shortk.hip", "attention_gemm.hip", "elementwise.hip", "sampler_step.hip", "rng.hip", "guide_f32.hip", "weights.cpp", "ops_abi.cpp",
           "engine_weights.cpp", "engine_graph.cpp", "engine_exec.cpp", "engine.cpp"]
# -amdgpu-mfma-vgpr-form: keep MFMA accumulators in VGPRs. With the default heuristic the attention kernels put them in AccVGPRs
# and paid 144 v_accvgpr_read/write per KV tile to run the softmax on them (found in the ISA; attention family 475 -> see DESIGN.md)
FLAGS = ["--offload-arch=gfx950", "-O3", "-mllvm", "-amdgpu-mfma-vgpr-form=1"] + os.environ.get("DD_EXTRA_CFLAGS", "").split() + ["-std=c++17", "-fPIC", "-x", "hip", "-Wno-unused-result", "-Wno-c++20-designator",
         "-I", os.path.join(HERE, "..", "include")]


# per-file switches.  gemm_ws.hip: the SLP vectoriser turns the GEGLU / LayerNorm-fold epilogue into v_pk_fma_f32 / v_pk_mul_f32, which
# cost more issue time beside MFMAs than the scalar pairs they replace (MI355X guide, cycle constants)
# rng.hip: no contraction -- the fused add_noise must round exactly like the generator followed by add_noise's own kernel
PER_FILE = {"gemm_ws.hip": ["-fno-slp-vectorize"], "rng.hip": ["-ffp-contract=off"]}


def _newer(src, dst):
    if not os.path.exists(dst):
        return True
    t = os.path.getmtime(dst)
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    deps += [os.path.join(HERE, "..", "include", f) for f in os.listdir(os.path.join(HERE, "..", "include"))]
    return any(os.path.getmtime(d) > t for d in deps)


# The variants of the library: (name, object directory, library, extra flags).  The fp16 library is the same SOURCES compiled with
# -DDD_ACT_F16 (csrc/common.h: IEEE half instead of bf16 as the 16-bit storage format); an engine is a bf16 or an fp16 engine by the
# library it was created in (_lib.lib(act_dtype)).  DD_BUILD_OBJ / DD_BUILD_LIB move the bf16 variant alone.
LIB_F16 = os.path.join(HERE, "libdistdiff_hip_f16.so")
VARIANTS = [("bf16", OBJ, LIB, []), ("fp16", os.path.join(HERE, "csrc", "_obj_f16"), LIB_F16, ["-DDD_ACT_F16"])]


def build(force=False, verbose=True):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    srcs = [s for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]
    jobs = []
    for name, objdir, _, extra in VARIANTS:
        os.makedirs(objdir, exist_ok=True)
        for s in srcs:
            src = os.path.join(CSRC, s)
            obj = os.path.join(objdir, s + ".o")
            if force or _newer(src, obj):
                jobs.append((name, src, obj, extra))

    def cc(job):
        name, src, obj, extra = job
        cmd = [hipcc] + FLAGS + extra + PER_FILE.get(os.path.basename(src), []) + ["-c", src, "-o", obj]
        if verbose:
            print("[build]", name, os.path.basename(src), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed for %s (%s):\n%s" % (src, name, r.stderr[-4000:]))
        return obj

    # eight compilers: both variants in the wall time one took on four
    with ThreadPoolExecutor(max_workers=8) as ex:
        list(ex.map(cc, jobs))
    for name, objdir, lib, _ in VARIANTS:
        objs = [os.path.join(objdir, s + ".o") for s in srcs]
        if force or any(j[0] == name for j in jobs) or not os.path.exists(lib):
            cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError("link failed (%s):\n%s" % (name, r.stderr[-4000:]))
            if verbose:
                print("[build] linked", lib, flush=True)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
