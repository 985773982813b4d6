"""CPU checks of the CFG-free mode (dd_set_cfg_free: one UNet pass per step, on the conditional prompt alone).  The plan of a CFG-free
engine through dd_debug_plan_only (fake device addresses, no GPU), the state machine of the two new engine entry points, the refusals,
the ABI surface (version still 11, argument counts of header and ctypes mirrors) and the CLI flag.  The GPU side is
tests/test_cfg_free_gpu.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_engine_plans as M  # noqa: E402

K = {n: i for i, n in enumerate(M.OP_KINDS)}
OF = {n: i for i, n in enumerate(M.OP_FIELDS)}
TF = {n: i for i, n in enumerate(M.TENSOR_FIELDS)}
PF = {n: i for i, n in enumerate(M.PROGRAM_FIELDS)}
DD_ERR_STATE = -3
NEW = {"dd_set_cfg_free": "distdiff_hip.h", "dd_cfg_free": "distdiff_hip.h", "dd_op_sampler_step1": "distdiff_hip_ops.h",
       "dd_op_sampler_step1_bwd": "distdiff_hip_ops.h"}


def planned(L, model, cfg_free, finalize=True):
    """An engine that only plans (make_engine_plans.plan with dd_set_cfg_free between create and finalize) -> (handle, config, rc of
    dd_finalize_weights)."""
    from distdiff_amd.engine import _to_c_config
    from distdiff_amd.weights import synthetic_weights
    cfg = M._config(model)
    with torch.device("meta"):
        w = synthetic_weights(cfg, seed=0, num_classes=5)
    h = C.c_void_p()
    cc = _to_c_config(cfg, 1, 2)
    assert L.dd_create(C.byref(cc), C.byref(h)) == 0
    assert L.dd_debug_plan_only(h) == 0
    if cfg_free is not None:
        assert L.dd_set_cfg_free(h, int(cfg_free)) == 0
    for model_name in ("unet", "vae", "guide"):
        for key, t in w[model_name].items():
            if key.startswith(("fc.", "classifier.")) or key.endswith("num_batches_tracked"):
                continue
            shape = (C.c_int64 * t.dim())(*t.shape)
            assert L.dd_declare_tensor(h, model_name.encode(), key.encode(), t.dim(), shape) == 0
    return h, cfg, (L.dd_finalize_weights(h) if finalize else None)


def unet_plan(L, h):
    n = L.dd_debug_plan_dump(h, 0, None, 0)
    assert n > 0
    a = np.zeros(n, np.int64)
    assert L.dd_debug_plan_dump(h, 0, a.ctypes.data_as(C.c_void_p), n) == n
    nt, nops = int(a[0]), int(a[1])
    nh, tw, ow = len(M.PROGRAM_FIELDS), len(M.TENSOR_FIELDS), len(M.OP_FIELDS)
    assert len(a) == nh + nt * tw + nops * ow
    return a[:nh], a[nh:nh + nt * tw].reshape(nt, tw), a[nh + nt * tw:].reshape(nops, ow)


def test_plan_of_a_cfg_free_engine(hip_lib):
    L = hip_lib
    h1, cfg, rc = planned(L, "tiny", True)
    assert rc == 0, L.dd_last_error(h1).decode()
    h2, _, rc = planned(L, "tiny", None)
    assert rc == 0
    try:
        head1, t1, ops1 = unet_plan(L, h1)
        head2, t2, ops2 = unet_plan(L, h2)
        # the default plan duplicates at the first cross-attention and ends on 2B images; the CFG-free one never does
        assert (ops2[:, OF["kind"]] == K["DUP"]).any() and set(t2[:, TF["B"]].tolist()) == {cfg.max_batch, 2 * cfg.max_batch}
        assert not (ops1[:, OF["kind"]] == K["DUP"]).any()
        assert set(t1[:, TF["B"]].tolist()) == {cfg.max_batch}
        for f in ("act_bytes", "grad_bytes"):
            assert 0 < head1[PF[f]] < head2[PF[f]], (f, head1[PF[f]], head2[PF[f]])
        assert L.dd_workspace_bytes(h1) < L.dd_workspace_bytes(h2)
        # the same layers in the same order, minus the duplications
        assert ops1[:, OF["kind"]].tolist() == [k for k in ops2[:, OF["kind"]].tolist() if k != K["DUP"]]
        # dd_set_cfg_free(0) after the default is the default engine, and an engine that was never told is the recorded plan
        rec = M.load()
        assert (rec["tiny/programs"][0] == head2).all()
    finally:
        L.dd_destroy(h1)
        L.dd_destroy(h2)


def test_set_cfg_free_is_a_setting_until_finalize(hip_lib):
    L = hip_lib
    h, _, _ = planned(L, "tiny", None, finalize=False)
    try:
        assert L.dd_cfg_free(h) == 0
        assert L.dd_set_cfg_free(h, 1) == 0 and L.dd_cfg_free(h) == 1
        assert L.dd_set_cfg_free(h, 0) == 0 and L.dd_cfg_free(h) == 0
        assert L.dd_set_cfg_free(h, 1) == 0
        assert L.dd_finalize_weights(h) == 0, L.dd_last_error(h).decode()
        assert L.dd_cfg_free(h) == 1
        assert L.dd_set_cfg_free(h, 0) == DD_ERR_STATE and b"dd_finalize_weights" in L.dd_last_error(h)
        assert L.dd_set_cfg_free(h, 1) == DD_ERR_STATE
        assert L.dd_cfg_free(h) == 1
    finally:
        L.dd_destroy(h)
    assert L.dd_set_cfg_free(None, 1) == -1 and L.dd_cfg_free(None) == -1      # DD_ERR_ARG


def test_sdxl_is_refused_at_finalize(hip_lib):
    L = hip_lib
    h, _, rc = planned(L, "tiny_sdxl", True)
    try:
        msg = L.dd_last_error(h).decode()
        assert rc != 0 and "cfg_free" in msg and "text_time" in msg, (rc, msg)
    finally:
        L.dd_destroy(h)
    h, _, rc = planned(L, "tiny_sdxl", False)      # and only with the flag
    assert rc == 0
    L.dd_destroy(h)


def _prototype(header, name):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b(?:int|float|size_t)\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, "%s is not declared in include/%s" % (name, header)
    return [a.strip() for a in m.group(1).split(",")]


def test_abi_version_and_argument_counts(hip_lib):
    from distdiff_amd import _lib
    L = hip_lib
    assert L.dd_abi_version() == 11 == _lib.ABI_VERSION
    assert sorted(NEW) == sorted(_lib.CFG_FREE_SYMBOLS)
    for name, header in NEW.items():
        assert name in (_lib.ENGINE_SYMBOLS if header == "distdiff_hip.h" else _lib.OPS_SYMBOLS)
        assert len(_prototype(header, name)) == len(getattr(L, name).argtypes), name
    # dd_op_sampler_step1 is dd_op_sampler_step_2m_n without (guidance_rescale, stats, part), the backward likewise without m2 as well
    assert len(_prototype("distdiff_hip_ops.h", "dd_op_sampler_step1")) == len(_prototype("distdiff_hip_ops.h", "dd_op_sampler_step_2m_n")) - 3
    assert len(_prototype("distdiff_hip_ops.h", "dd_op_sampler_step1_bwd")) == len(_prototype("distdiff_hip_ops.h", "dd_op_sampler_step_bwd")) - 4


def test_a_library_without_the_symbols_is_refused_only_when_asked(hip_lib):
    from distdiff_amd import _lib

    class Old:      # a library built before the mode: everything but the four symbols
        def __getattr__(self, name):
            if name in _lib.CFG_FREE_SYMBOLS:
                raise AttributeError(name)
            return getattr(hip_lib, name)

    with pytest.raises(_lib.DistDiffLibraryError, match="CFG-free.*dd_set_cfg_free"):
        _lib.require_cfg_free(Old())
    _lib.require_cfg_free(hip_lib)


def test_cli_flag():
    from distdiff_amd import generate_data as G
    base = ["--synthetic", "4", "--tiny", "--output_dir", "unused"]
    assert G.parse_args(base).cfg_free is False
    a = G.parse_args(base + ["--cfg_free", "--guidance_scale", "1.0"])
    assert a.cfg_free is True and a.guidance_rescale == 0.0
    with pytest.raises(SystemExit, match="--cfg_free.*--guidance_rescale"):
        G.parse_args(base + ["--cfg_free", "--guidance_rescale", "0.5"])
    with pytest.raises(SystemExit, match="--cfg_free.*sdxl"):
        G.parse_args(base + ["--cfg_free", "--synthetic_arch", "sdxl"])
    assert G.parse_args(base + ["--guidance_rescale", "0.5"]).guidance_rescale == 0.5      # without the flag: as before
    with pytest.raises(SystemExit, match="always runs classifier-free guidance"):         # the existing refusal stays
        G.parse_args(base + ["--do_classifier_free_guidance", ""])
