"""CPU checks of the fp16 variant of the library (libdistdiff_hip_f16.so: the same sources compiled with -DDD_ACT_F16): both libraries in
one process, the host weight packer's fp32 -> half rounding, the planners (the storage format must not move a problem to another kernel;
the fp16 library refuses fp8 P.V) and the CLI flag.  No device is touched."""
import ctypes

import numpy as np
import pytest
import torch

import attention_plan_cases as acases
import conv_plan_cases as ccases


@pytest.fixture(scope="module")
def libs():
    import __graft_entry__ as g
    g.build()
    from distdiff_amd import _lib
    return _lib.lib("bf16"), _lib.lib("fp16")


def test_both_libraries_load_in_one_process(libs):
    from distdiff_amd import _lib
    bf, h = libs
    assert bf is not h and bf is _lib.lib() and h is _lib.lib(torch.float16) and bf is _lib.lib(torch.bfloat16)
    assert (bf.dd_act_dtype(), h.dd_act_dtype()) == (0, 1)
    assert bf.dd_abi_version() == h.dd_abi_version() == _lib.ABI_VERSION == 11
    with pytest.raises(ValueError):
        _lib.lib(torch.float32)


def test_a_library_of_the_other_format_is_refused(libs, monkeypatch):
    from distdiff_amd import _lib
    monkeypatch.setattr(_lib, "_lib_f16", None)
    monkeypatch.setattr(_lib, "LIB_PATH_F16", _lib.LIB_PATH)           # the bf16 library where the fp16 one is expected
    with pytest.raises(_lib.DistDiffLibraryError, match="stores bf16"):
        _lib.lib("fp16")


SPECIAL = np.array([
    1.0, -1.0, 0.0, -0.0, 65504.0, -65504.0, 65519.99, 65520.0, -65520.0, 65536.0, 1e9, np.inf, -np.inf, np.nan,
    1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20, 1.0 + 2.0 ** -11 - 2.0 ** -20,       # ties to even / to odd, and beside them
    2048.0 + 1.0, 2048.0 + 3.0, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 + 2.0 ** -40, 3 * 2.0 ** -25,
    2.0 ** -26, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 1023.5 * 2.0 ** -24, 1023.75 * 2.0 ** -24, 6.1e-5, -3.3e-6, 1e-8, 1e-30,
], dtype=np.float32)


def test_host_packer_rounds_to_nearest_even_half(libs):
    """dd_pack_conv_weight of the fp16 library (through ops.PackedConv, as every caller packs) against numpy's float32 -> float16, bit for bit:
    ties, the largest normal, 65520 -> inf, subnormals, signed zeros, inf; NaN stays NaN.  Plus 20000 random bit patterns."""
    from distdiff_amd import ops
    rng = np.random.default_rng(3)
    rand = rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    vals = np.concatenate([SPECIAL, rand])
    n = len(vals) // 8 * 8
    w = torch.from_numpy(vals[:n].copy()).reshape(1, n)
    with np.errstate(over="ignore"):
        want = vals[:n].astype(np.float16)
    for mode in (0, 1):
        pk = ops.PackedConv(w if mode == 0 else w.t().contiguous(), 0, mode=mode, device="cpu", dtype=torch.float16)
        assert pk.w.dtype == torch.float16 and (pk.N, pk.cin) == (1, n)
        got = pk.w.view(torch.int16).numpy().view(np.uint16).reshape(-1)[:n]
        nan = np.isnan(want)
        assert np.array_equal(got[~nan], want.view(np.uint16)[~nan])
        assert np.isnan(got.view(np.float16)[nan]).all() and nan.sum() >= 1
    # the bf16 library packs bf16, as before
    pk = ops.PackedConv(w, 0, device="cpu")
    ok = ~np.isnan(vals[:n])
    assert pk.w.dtype == torch.bfloat16 and torch.equal(pk.w.reshape(-1)[:n][torch.from_numpy(ok)], w.reshape(-1).to(torch.bfloat16)[torch.from_numpy(ok)])


def test_conv_planner_does_not_depend_on_the_storage_format(libs):
    from distdiff_amd import _lib
    rng = np.random.default_rng(5)
    n = 0
    for name, rows in ccases.blocks():
        pick = rows[rng.choice(len(rows), size=min(len(rows), 400), replace=False)]
        a, b = ccases.evaluate(_lib.LIB_PATH, pick), ccases.evaluate(_lib.LIB_PATH_F16, pick)
        assert np.array_equal(a, b), name
        n += len(pick)
    assert n > 2000


def test_attention_planner_refuses_fp8_and_is_otherwise_the_same(libs):
    from distdiff_amd import _lib
    rng = np.random.default_rng(7)
    fp8_rows = 0
    for name, rows in acases.blocks():
        pick = rows[rng.choice(len(rows), size=min(len(rows), 400), replace=False)]
        a, b = acases.evaluate(_lib.LIB_PATH, pick), acases.evaluate(_lib.LIB_PATH_F16, pick)
        fp8 = pick[:, acases.COL["fp8"]] != 0
        assert np.array_equal(a[~fp8], b[~fp8]), name
        assert (b[fp8, 0] == -1).all(), name                     # route -1: refused
        fp8_rows += int(((a[:, 0] >= 0) & fp8).sum())
    assert fp8_rows > 0                                          # ... problems the bf16 library does plan


def test_plan_queries_take_the_format(libs):
    from distdiff_amd import ops
    from distdiff_amd._lib import AttnParams
    p = AttnParams()
    p.q = p.k = p.v = p.o = p.lse = ctypes.c_void_p(4096)
    p.B, p.H, p.Nq, p.Nk, p.D, p.scale = 1, 2, 1024, 1024, 64, 0.125
    p.ldq = p.ldk = p.ldv = p.ldo = 128
    assert ops._attention_plan(p, 0, False, torch.float16) == ops._attention_plan(p, 0, False)
    p.pv_fp8 = 1
    assert ops._attention_plan(p, 0, False)["fp8"]
    with pytest.raises(RuntimeError):
        ops._attention_plan(p, 0, False, torch.float16)
    w = torch.randn(160, 64, 3, 3)
    plans = [ops.conv_gemm_plan(None, ops.PackedConv(w, 1, device="cpu", dtype=dt), 6, 128, 128, 128, 128) for dt in (torch.bfloat16, torch.float16)]
    assert plans[0] == plans[1] and plans[0][0] == "conv_halo"


def test_cli_flag(monkeypatch):
    from distdiff_amd import engine, generate_data as G
    a = G.parse_args([])
    assert a.act_dtype == "bf16" and a.attn_fp8 is False
    assert G.parse_args(["--act_dtype", "fp16", "--mixed_precision", "bf16"]).act_dtype == "fp16"       # --mixed_precision: accepted, ignored
    with pytest.raises(SystemExit):
        G.parse_args(["--act_dtype", "fp16", "--attn_fp8"])
    with pytest.raises(SystemExit):
        G.parse_args(["--act_dtype", "fp32"])
    seen = []

    class Fake:
        def __init__(self, cfg, weights, **kw):
            seen.append(kw)

        def set_schedule(self, *a, **kw):
            pass
    monkeypatch.setattr(engine, "Engine", Fake)
    base = ["--synthetic", "2", "--tiny", "--engine_batch", "2", "--steps", "4"]
    G.build_engine(G.parse_args(base), device="cpu")
    G.build_engine(G.parse_args(base + ["--act_dtype", "fp16"]), device="cpu")
    assert "act_dtype" not in seen[0] and seen[1]["act_dtype"] == "fp16"      # the default call is the call it was


def test_engine_refuses_fp16_with_fp8_attention_before_any_device_call():
    from distdiff_amd.config import tiny_config
    from distdiff_amd.engine import DDConfig, Engine
    from distdiff_amd import _lib
    with pytest.raises(ValueError):
        Engine(tiny_config(max_batch=1), {}, act_dtype="fp16", attn_fp8=True, device="cpu")
    # and the library itself: dd_create of the fp16 library returns DD_ERR_ARG for unet_attn_fp8
    cfg = DDConfig()
    cfg.max_batch, cfg.abi_version, cfg.unet_attn_fp8 = 1, _lib.ABI_VERSION, 1
    h = ctypes.c_void_p()
    assert _lib.lib("fp16").dd_create(ctypes.byref(cfg), ctypes.byref(h)) == -1 and not h.value
    assert _lib.lib("bf16").dd_create(ctypes.byref(cfg), ctypes.byref(h)) == 0 and h.value
    _lib.lib("bf16").dd_destroy(h)
