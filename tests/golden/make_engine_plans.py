"""Records the engine's plans -- every tensor and op of the six programs, the program and workspace totals and the packed-weight layout --
for every configuration of CASES into tests/golden/engine_plans.npz.  No GPU: dd_debug_plan_only makes dd_finalize_weights build and
plan an engine on fake device addresses, dd_debug_plan_dump writes the plans as int64 words (include/distdiff_hip_ops.h).

    python tests/golden/make_engine_plans.py

The committed table was recorded at commit de4e83d ("Big conv/GEMM kernel: one tile description, one dispatcher, bits pinned") with only
these two hooks applied -- they are additive: dmalloc / wupload take another branch, nothing that plans does -- BEFORE the graph, engine
object and plan switches were reorganised: it pins what that commit planned, so that the refactor (and every later change that does not
mean to move a plan) can be checked record by record on a CPU.  Re-record only when a plan is changed on purpose, and say which.

Weights are never materialised: the state dicts are built under torch.device("meta") and declared by shape (dd_declare_tensor).
Every case runs in a process of its own (at the recorded commit DD_NO_LN_FOLD was read once per process).

The file holds per case `<case>/engine` (total_bytes, partial_cap, tmp_cap, the count and the sizes of the packed weight buffers in
order), `<case>/programs` (int64 [6, 9]: PROGRAM_FIELDS of unet, vae, guide, vae encoder, text, text2) and either `<case>/tensors<p>` /
`<case>/ops<p>` (int64 [n, 16] / [n, 50], TENSOR_FIELDS / OP_FIELDS) for every program p, or, where those exceed 256 KB compressed,
`<case>/sha256` (one digest per program over its tensor and op words).
"""
import hashlib
import io
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
PATH = os.path.join(HERE, "engine_plans.npz")
RAW_LIMIT = 256 * 1024

PROGRAMS = ("unet", "vae", "guide", "venc", "text", "text2")
PROGRAM_FIELDS = ("tensors", "ops", "act_bytes", "grad_bytes", "scratch_partial", "scratch_tmp", "scratch_rowpart", "tr_max", "tr_count")
TENSOR_FIELDS = ("off", "goff", "parent", "rows", "C", "ld", "B", "H", "W", "f32", "grad", "gf32", "transient", "tr_slot", "glo", "ghi")
OP_FIELDS = ("kind", "x", "y", "res", "raw", "q", "k", "v", "x2", "cw", "nw", "stride", "up", "relu", "out_f32", "use_table", "G", "silu",
             "eps", "heads", "D", "Nq", "Nk", "cross_slot", "causal", "act_kind", "pv_fp8", "q_prescaled", "patch", "sel_stride", "stats_off",
             "fused", "x_acc", "res_acc", "x2_acc", "res_alias", "part", "part_off", "part_ld", "n_producers", "producers_hash", "gn_fused",
             "ln_fold", "x_fwd", "ln_stats_off", "rowstat_from", "rowstat_emit", "rowstat_ld", "row_spans", "flops")
OP_KINDS = ("CONV", "GN", "LN", "ATTN", "CONCAT", "MAXPOOL", "ACT", "PATCHIFY", "VITEMBED", "SELECT", "DUP")
SWITCHES = ("DD_NO_LN_FOLD", "DD_NO_LN_ROWSTATS", "DD_NO_GN_FUSION", "DD_NO_CONCAT_FUSION", "DD_NO_GRAD_ALIAS", "DD_NO_TRANSIENT",
            "DD_NO_CFG_SHARE", "DD_NO_GRAD_REUSE")
VIT = dict(kind="vit", input_size=64, vit_width=64, vit_layers=2, vit_heads=2, vit_patch=16, vit_mlp=128, vit_out=32)
MBV2 = dict(kind="mbv2", input_size=64, mb_stem=16, mb_channels=(16, 16, 32), mb_repeats=(1, 2, 2), mb_strides=(1, 2, 2), mb_expand=2, mb_head=64)


def _config(model):
    from distdiff_amd import config as K
    if model == "tiny":
        return K.tiny_config(max_batch=2)
    if model == "tiny_sdxl":
        return K.tiny_sdxl_config(max_batch=2)
    if model in ("tiny_vit", "tiny_mbv2"):
        cfg = K.tiny_config(max_batch=2)
        cfg.guide = K.GuideConfig(**(VIT if model == "tiny_vit" else MBV2))
        return cfg
    if model == "wide128":      # tests/test_engine_gpu.py::test_fusion_plan_is_fixed_at_finalize
        cfg = K.tiny_config(latent_size=64, max_batch=4)
        cfg.unet = K.UNetConfig(block_out_channels=(128, 128, 128, 128), layers_per_block=1, num_heads=2, cross_attention_dim=64, norm_num_groups=8)
        return cfg
    if model.startswith("sd15_"):      # sd15_L<latent>_B<batch>
        L, B = (int(x[1:]) for x in model.split("_")[1:])
        return K.sd15_config(latent_size=L, max_batch=B)
    if model == "sd21":
        return K.sd21_config(latent_size=96, max_batch=2)
    if model == "sdxl":
        return K.sdxl_config(latent_size=128, max_batch=8)
    raise KeyError(model)


def _cases():
    c = {}

    def add(name, model, grad=1, encoders=False, act="bf16", env=None):
        c[name] = dict(model=model, grad=grad, encoders=encoders, act=act, env=env)

    add("tiny", "tiny")
    add("tiny_nograd", "tiny", grad=0)
    add("tiny_sdxl_enc", "tiny_sdxl", encoders=True)
    add("tiny_vit", "tiny_vit")
    add("tiny_mbv2", "tiny_mbv2")
    add("wide128", "wide128")
    add("sd15_L32_B2", "sd15_L32_B2")
    add("sd15_L64_B32", "sd15_L64_B32")      # the bench workload
    add("sd15_L96_B8", "sd15_L96_B8")
    add("sd21", "sd21", encoders=True)
    add("sdxl_B8", "sdxl", encoders=True)
    for sw in SWITCHES:
        add("tiny/" + sw, "tiny", env=sw)
        add("sd15_L64_B32/" + sw, "sd15_L64_B32", env=sw)
    add("tiny_f16", "tiny", act="fp16")
    add("sd15_L64_B32_f16", "sd15_L64_B32", act="fp16")
    return c


CASES = _cases()


def plan(name):
    """The plans of case `name` on the library of this tree -> {"engine", "programs", "tensors<p>", "ops<p>"} of int64 arrays.  The plan
    switch of the case is in the environment while the engine is created and finalized, and only then."""
    import ctypes as C
    import torch
    from distdiff_amd import _lib
    from distdiff_amd.engine import _to_c_config
    from distdiff_amd.weights import synthetic_weights
    case = CASES[name]
    cfg = _config(case["model"])
    with torch.device("meta"):
        w = synthetic_weights(cfg, seed=0, num_classes=5, encoders=case["encoders"])
    L = _lib.lib(case["act"])
    h = C.c_void_p()
    old = {sw: os.environ.pop(sw, None) for sw in SWITCHES}
    if case["env"]:
        os.environ[case["env"]] = "1"
    try:
        cc = _to_c_config(cfg, case["grad"], 2)
        assert L.dd_create(C.byref(cc), C.byref(h)) == 0
        assert L.dd_debug_plan_only(h) == 0
        for model in ("unet", "vae", "guide", "text", "text2"):
            for key, t in w.get(model, {}).items():
                if key.startswith(("fc.", "classifier.")) or key.endswith("num_batches_tracked"):
                    continue
                shape = (C.c_int64 * t.dim())(*t.shape)
                assert L.dd_declare_tensor(h, model.encode(), key.encode(), t.dim(), shape) == 0
        rc = L.dd_finalize_weights(h)
        assert rc == 0, L.dd_last_error(h).decode()
    finally:
        os.environ.pop(case["env"] or "", None)
        os.environ.update({k: v for k, v in old.items() if v is not None})

    def words(prog):
        n = L.dd_debug_plan_dump(h, prog, None, 0)
        assert n >= 0
        a = np.zeros(n, np.int64)
        assert L.dd_debug_plan_dump(h, prog, a.ctypes.data_as(C.c_void_p), n) == n
        return a

    out = {"engine": words(6)}
    assert out["engine"][0] == L.dd_workspace_bytes(h) and out["engine"][3] == len(out["engine"]) - 4
    heads = []
    for p in range(6):
        a = words(p)
        nt, nops = int(a[0]), int(a[1])
        nh, tw, ow = len(PROGRAM_FIELDS), len(TENSOR_FIELDS), len(OP_FIELDS)
        assert len(a) == nh + nt * tw + nops * ow
        heads.append(a[:nh])
        out["tensors%d" % p] = a[nh:nh + nt * tw].reshape(nt, tw)
        out["ops%d" % p] = a[nh + nt * tw:].reshape(nops, ow)
    out["programs"] = np.stack(heads)
    # every launching entry point refuses an engine that only plans
    assert L.dd_set_prototypes(h, None, None, 1, 1, 1) == -3 and L.dd_decode(h, C.c_void_p(8), C.c_void_p(8), 0, cfg.max_batch, None) == -3      # DD_ERR_STATE
    L.dd_destroy(h)
    return out


def digests(got):
    return np.array([hashlib.sha256(got["tensors%d" % p].tobytes() + got["ops%d" % p].tobytes()).hexdigest() for p in range(6)])


def load():
    with np.load(PATH) as f:
        return {k: f[k] for k in f.files}


def _compressed_size(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.tell()


def main():
    sys.path.insert(0, ROOT)
    if "--case" in sys.argv:      # the process of one case: its arrays to the given file
        name, path = sys.argv[sys.argv.index("--case") + 1:][:2]
        np.savez(path, **plan(name))
        return
    import tempfile
    tmp = tempfile.mkdtemp()

    def run(item):
        i, name = item
        path = os.path.join(tmp, "%d.npz" % i)
        subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, path], check=True)
        with np.load(path) as f:
            return name, {k: f[k] for k in f.files}

    with ThreadPoolExecutor(4) as ex:
        results = dict(ex.map(run, enumerate(CASES)))
    rec, report = {}, {}
    for name in CASES:
        got = results[name]
        rec[name + "/engine"], rec[name + "/programs"] = got["engine"], got["programs"]
        raw = {"%s/%s" % (name, k): v for k, v in got.items() if k.startswith(("tensors", "ops"))}
        size = _compressed_size(raw)
        if size > RAW_LIMIT:
            rec[name + "/sha256"] = digests(got)
        else:
            rec.update(raw)
        report[name] = dict(kb=size // 1024, raw=size <= RAW_LIMIT, unet_ops=int(got["programs"][0][1]), total_gb=round(int(got["engine"][0]) / 1e9, 3))
    np.savez_compressed(PATH, **rec)
    print(json.dumps(report, indent=1))
    print("wrote %s: %d cases, %d bytes" % (PATH, len(CASES), os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
