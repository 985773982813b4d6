"""The case table of the exact-input tests of the conv / GEMM kernels, and the one function that turns a case into the arguments of
ops.conv_gemm / ops.conv_gemm_plan.  No device is needed to import this or to ask the planner (tests/test_conv_exact_cases.py walks the
table on the CPU); tests/test_conv_exact_gpu.py runs it.

A case is (Problem, plan, f16): the problem in the terms of tests/exact_ref.py, the (kind, form, split) the launcher must give it, and
whether the fp16 library runs it too (one case per kind and form).  The shapes are the smallest the planner routes as stated; tuples in
the comments are (B, Cin, Cout, H, W).  Halo kinds need M >= 49152 rows.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_conv_big_bits as big  # noqa: E402
import make_pingpong_bits as pp  # noqa: E402
from exact_ref import Problem, pad8, stored_width, store_dtype  # noqa: E402

G, HALO, PERSIST, WS, PPS = "general", "conv_halo", "conv_halo_persist", "gemm_ws", "gemm_pps"
S128, S256 = "small_128x128", "small_256x64"
F1, F2, F3, F4, F5 = big.F1, big.F2, big.F3, big.F4, big.F5


def conv(name, B, Cin, Cout, H, W, plan, f16=False, **kw):
    return Problem(name, B, Cin, Cout, H, W, **kw), plan, f16


def gemm(name, M, K, N, plan, f16=False, **kw):
    return Problem(name, 1, K, N, M, 1, k=1, **kw), plan, f16


CASES = [
    # ---- the small kernel (conv_gemm_kernel), automatic split ----
    conv("small_3x3_c64", 2, 64, 128, 16, 16, (G, S128, 2), f16=True),
    conv("small_3x3_c64_dgrad", 2, 64, 128, 16, 16, (G, S256, 4), f16=True, dgrad=True, fl=""),
    conv("small_3x3_cin4", 2, 4, 64, 16, 16, (G, S256, 1)),
    conv("small_3x3_cin4_dgrad", 2, 4, 64, 16, 16, (G, S256, 2), dgrad=True, fl=""),
    conv("small_3x3_cin40_ragged_m63", 1, 40, 72, 9, 7, (G, S128, 1)),
    conv("small_3x3_cin40_ragged_m63_dgrad", 1, 40, 72, 9, 7, (G, S128, 2), dgrad=True, fl=""),
    conv("small_7x7_stride2_stem", 1, 3, 64, 32, 32, (G, S256, 1), k=7, stride=2),
    conv("small_7x7_stride2_stem_dgrad", 1, 3, 64, 32, 32, (G, S256, 10), k=7, stride=2, dgrad=True, fl=""),
    conv("small_1x1_stride2", 2, 64, 128, 8, 8, (G, S128, 1), k=1, stride=2),
    conv("small_1x1_stride2_dgrad", 2, 64, 128, 8, 8, (G, S128, 1), k=1, stride=2, dgrad=True, fl=""),
    conv("small_3x3_deepK_split15", 2, 1280, 128, 8, 8, (G, S128, 15)),
    conv("small_3x3_stride2", 2, 64, 64, 16, 16, (G, S128, 2), stride=2),
    conv("small_3x3_stride2_dgrad", 2, 64, 64, 16, 16, (G, S256, 2), stride=2, dgrad=True, fl=""),
    conv("small_3x3_up2", 2, 64, 64, 8, 8, (G, S256, 2), up=1),
    conv("small_3x3_up2_dgrad", 2, 64, 64, 8, 8, (G, S256, 2), up=1, dgrad=True, fl=""),
    # ---- conv_gemm_big_kernel, every form (ksplit = 1 but for the split-K case) ----
    conv("big_128x256", 2, 512, 256, 24, 24, (G, F1, 1), f16=True, ksplit=1),
    conv("big_128x256_dgrad", 2, 512, 256, 24, 24, (G, F1, 1), dgrad=True, fl="", ksplit=1),
    conv("big_128x256_res_relu_mask", 2, 512, 256, 24, 24, (G, F1, 1), fl="brum", ksplit=1),
    conv("big_128x256_res_f32", 2, 512, 256, 24, 24, (G, F1, 1), fl="bR", ksplit=1),
    conv("big_128x256_f32_out_alpha", 2, 512, 256, 24, 24, (G, F1, 1), fl="bfa", ksplit=1),
    conv("big_256x128", 2, 512, 128, 32, 32, (G, F3, 1), f16=True, ksplit=1),
    conv("big_256x128_dgrad_128x128_two_workgroups", 2, 512, 128, 32, 32, (G, F5, 1), dgrad=True, fl="", ksplit=1),
    conv("big_128x160_two_workgroups_ragged_m", 2, 320, 320, 24, 25, (G, F4, 1), f16=True, ksplit=1),
    conv("big_128x160_two_workgroups_ragged_m_dgrad", 2, 320, 320, 24, 25, (G, F4, 1), dgrad=True, fl="", ksplit=1),
    conv("big_128x160_two_workgroups_pointwise", 4, 1280, 320, 32, 32, (G, F4, 1), k=1, ksplit=1),
    conv("big_128x160_two_workgroups_pointwise_dgrad", 4, 1280, 320, 32, 32, (G, F4, 1), k=1, dgrad=True, fl="", ksplit=1),
    conv("big_128x128_two_workgroups_ragged", 3, 128, 384, 20, 21, (G, F5, 1), f16=True, ksplit=1),
    conv("big_256x160_splitk15", 2, 1280, 320, 24, 24, (G, F2, 15), f16=True),
    conv("big_256x160", 2, 1280, 320, 24, 24, (G, F2, 1), ksplit=1),
    conv("big_256x160_dgrad_128x160_two_workgroups_splitk4", 2, 1280, 320, 24, 24, (G, F4, 4), dgrad=True, fl=""),
    # split-K of the other forms (a caller's ksplit: the automatic split gives these shapes to the small kernel)
    conv("big_128x256_splitk3", 2, 512, 256, 24, 24, (G, F1, 3), ksplit=3),
    conv("big_256x128_splitk2", 2, 512, 128, 32, 32, (G, F3, 2), ksplit=2),
    conv("big_128x128_two_workgroups_splitk2_res_relu", 3, 128, 384, 20, 21, (G, F5, 2), fl="bru", ksplit=2),
    # ---- conv_halo_kernel ----
    conv("halo_320_32x32", 48, 320, 320, 32, 32, (HALO, None, 1), f16=True),
    conv("halo_320_32x32_dgrad", 48, 320, 320, 32, 32, (HALO, None, 1), dgrad=True, fl=""),
    conv("halo_320_32x32_res_relu", 48, 320, 320, 32, 32, (HALO, None, 1), fl="bru"),
    # a mask, an fp32 residual, fp32 output or alpha != 1: the planner gives the problem to the general forms
    conv("halo_320_32x32_res_relu_mask_goes_general", 48, 320, 320, 32, 32, (G, F4, 1), fl="brum"),
    conv("halo_320_32x32_res_f32_goes_general", 48, 320, 320, 32, 32, (G, F4, 1), fl="bR"),
    conv("halo_320_32x32_f32_out_alpha_goes_general", 48, 320, 320, 32, 32, (G, F4, 1), fl="bfa"),
    conv("halo_640_16x16", 192, 128, 640, 16, 16, (HALO, None, 1)),
    conv("halo_up2_320", 24, 128, 320, 32, 32, (HALO, None, 1), up=1),
    conv("halo_w48", 24, 64, 320, 48, 48, (HALO, None, 1)),
    conv("halo_w80", 8, 128, 320, 80, 80, (HALO, None, 1)),
    conv("halo_w96", 6, 320, 320, 96, 96, (HALO, None, 1)),
    conv("halo_w96_dgrad", 6, 320, 320, 96, 96, (HALO, None, 1), dgrad=True, fl=""),
    conv("halo_8x8_cin2560_split8", 32, 2560, 1280, 8, 8, (HALO, None, 8)),
    conv("halo_8x8_cin2560_split8_dgrad_split4", 32, 2560, 1280, 8, 8, (HALO, None, 4), dgrad=True, fl=""),
    conv("halo_8x8_cin2560_b16", 16, 2560, 1280, 8, 8, (HALO, None, 8)),
    conv("halo_8x8_cin1280_b4_split4", 4, 1280, 1280, 8, 8, (HALO, None, 4)),
    conv("halo_8x8_cin256_split2", 8, 256, 320, 8, 8, (HALO, None, 2), f16=True),
    conv("halo_narrow_n2_8_wide_rows", 8, 64, 2, 128, 128, (HALO, None, 1), f16=True, fl="bn", ksplit=1),
    conv("n4_f32_8_wide_rows_small_256x64", 16, 320, 4, 64, 64, (G, S256, 1), fl="bfn", ksplit=1),
    # ---- conv_halo_persist_kernel ----
    conv("persist_256_64x64", 12, 64, 256, 64, 64, (PERSIST, None, 1), f16=True),
    conv("persist_256_128x128", 3, 256, 256, 128, 128, (PERSIST, None, 1)),
    conv("persist_256_128x128_dgrad", 3, 256, 256, 128, 128, (PERSIST, None, 1), dgrad=True, fl=""),
    conv("persist_256_128x128_res_relu", 3, 256, 256, 128, 128, (PERSIST, None, 1), fl="bru"),
    conv("persist_256_128x128_res_relu_mask_goes_general", 3, 256, 256, 128, 128, (G, F1, 1), fl="brum"),
    conv("persist_256_128x128_res_f32_goes_general", 3, 256, 256, 128, 128, (G, F1, 1), fl="bR"),
    conv("persist_256_128x128_f32_out_alpha_goes_general", 3, 256, 256, 128, 128, (G, F1, 1), fl="bfa"),
    conv("persist_w256", 1, 64, 256, 256, 256, (PERSIST, None, 1)),
    conv("persist_n128_256x512", 1, 128, 128, 256, 512, (PERSIST, None, 1)),
    conv("persist_ragged_288_tiles", 9, 128, 128, 128, 128, (PERSIST, None, 1)),
    conv("persist_up2", 4, 128, 128, 128, 128, (PERSIST, None, 1), up=1),
    # ---- gemm_ws (K = 320) ----
    gemm("ws_n320_m33024", 33024, 320, 320, (WS, None, 1), f16=True, ksplit=1),
    gemm("ws_n640_m36928_relu", 36928, 320, 640, (WS, None, 1), fl="bu", ksplit=1),
    gemm("ws_n960_m33024_views", 33024, 320, 960, (WS, None, 1), fl="bv", ksplit=1),
    gemm("ws_n320_m36928_dgrad", 36928, 320, 320, (WS, None, 1), dgrad=True, fl="", ksplit=1),
    gemm("ws_n640_alpha", 36928, 320, 640, (WS, None, 1), fl="ba", ksplit=1),
    gemm("ws_n640_res_goes_general", 36928, 320, 640, (G, F4, 1), fl="br", ksplit=1),
    # ---- gemm_pps ----
    gemm("pps_n640_k1280", 49152, 1280, 640, (PPS, None, 1), f16=True, ksplit=1),
    gemm("pps_n640_k1280_res", 49152, 1280, 640, (PPS, None, 1), fl="br", ksplit=1),
    gemm("pps_n640_k1280_res_relu_alpha", 49152, 1280, 640, (PPS, None, 1), fl="brua", ksplit=1),
    gemm("pps_n640_k1280_res_relu_mask_goes_general", 49152, 1280, 640, (G, F4, 1), fl="brum", ksplit=1),
    gemm("pps_n640_k1280_res_f32_goes_general", 49152, 1280, 640, (G, F4, 1), fl="bR", ksplit=1),
    gemm("pps_n640_k1280_f32_out_goes_general", 49152, 1280, 640, (G, F4, 1), fl="bf", ksplit=1),
    gemm("pps_geglu_raw_stash", 40960, 256, 512, (PPS, None, 1), fl="bg", ksplit=1),
]
NAMES = [c[0].name for c in CASES]
HALO_CASES = [c for c in CASES if c[1][0] in (HALO, PERSIST)]


def record_problems():
    """{"big:case" | "pp:case": (Problem, salt, rowstat span | 0, plan | kind index)} for every case of the two bit records, in the flag
    letters of exact_ref (G: GEGLU without the stash, l: CF_LNFOLD -- neither has a closed form for y)"""
    out = {}
    for name, kind, B, H, shift, Cout, Cin, mode, fl in pp.CONV:
        f = "".join(c for c in fl if c in "brsu") + ("fn" if "f" in fl else "") + ("n" if "n" in fl else "")
        out["pp:" + name] = (Problem(name, B, Cin, Cout, H, H, up=shift, dgrad=bool(mode), fl=f, ksplit=1 if ("f" in fl or "n" in fl) else 0),
                             pp.CASES.index(name) * 16, 0, kind)
    for name, M, K, N, geglu, fl in pp.GEMM:
        out["pp:" + name] = (Problem(name, 1, K, N, M, 1, k=1, fl=fl + ("G" if geglu and "g" not in fl else ""), ksplit=1), pp.CASES.index(name) * 16,
                             40, pp.PPS)
    for name, form, ksplit, M, K, N, geglu, fl in big.GEMM:
        out["big:" + name] = (Problem(name, 1, K, N, M, 1, k=1, fl=fl.replace("p", "") + ("G" if geglu and "g" not in fl else ""), ksplit=ksplit),
                              big.CASES.index(name) * 16, big.SPAN.get(form, 0), (G, form, ksplit))
    for name, form, B, H, stride, shift, _parity, Cout, Cin, mode, fl in big.CONV:
        if mode:
            p = Problem(name, B, Cin, Cout, 2 * H, 2 * H, stride=2, dgrad=True, fl=fl, ksplit=1)
        else:
            p = Problem(name, B, Cin, Cout, H, H, stride=stride, up=shift, fl=fl, ksplit=1)
        out["big:" + name] = (p, big.CASES.index(name) * 16, 0, (G, form, 1))
    return out


def closed_form_outputs(prob):
    """the outputs of a case that exact_ref derives: "raw" for the stash, "y" unless GELU or the LayerNorm fold is in it"""
    if "g" in prob.fl:
        return ["raw"]
    return [] if ("G" in prob.fl or "l" in prob.fl) else ["y"]


def launch_args(ops, prob, dtype=torch.bfloat16, inp=None, dev="cpu", rowspan=0):
    """(pk, x, kw, out): the packed weights, the input rows and the keywords of ops.conv_gemm / ops.conv_gemm_plan for one case, and
    `out`, the WHOLE buffer that is compared (the output with its NaN-prefilled spare columns; the raw stash for "g").  inp = None (the
    planner: it only tests pointers for null): buffers of the right shape that nobody reads."""
    fl = prob.fl
    full = (lambda shape, dt: torch.empty(shape, dtype=dt)) if inp is None else (lambda shape, dt: torch.full(shape, float("nan"), dtype=dt, device=dev))
    put = lambda t, dt: torch.empty(t, dtype=dt) if inp is None else t.to(dt).to(dev)
    w = torch.zeros((prob.Cout, prob.Cin, prob.k, prob.k)) if inp is None else inp["w"]
    bias = None
    if "b" in fl:
        bias = torch.zeros(prob.N) if inp is None else inp["bias"]
    pk = ops.PackedConv(w, prob.pad, mode=int(prob.dgrad), geglu="g" in fl or "G" in fl, bias=bias, device=dev, dtype=dtype)
    ih, iw = prob.in_hw
    m_in, cin = prob.B * ih * iw, pad8(prob.in_ch)
    assert pk.cin == cin and pk.N == prob.N, (prob.name, pk.cin, cin, pk.N, prob.N)
    kw = dict(prob.launch_kw, ksplit=prob.ksplit, relu="u" in fl, out_f32="f" in fl)
    if "a" in fl:
        kw["alpha"] = 0.5
    xs = full((m_in, cin + (64 if "v" in fl else 0)), dtype)
    x = xs[:, -cin:]
    if inp is not None:
        x.copy_(inp["x"].to(dtype))
    if "v" in fl:
        kw["x_ld"] = xs.stride(0)
    M, ncols = prob.M, prob.ncols
    ybuf = full((M, ncols if "g" in fl else stored_width(prob)), store_dtype(prob, dtype))
    kw["y"] = ybuf[:, :ncols]
    out = ybuf
    if "r" in fl or "R" in fl:
        kw["res"] = put((M, ncols) if inp is None else inp["res"], torch.float32 if "R" in fl else dtype)
    if "m" in fl:
        kw["mask"] = put((M, ncols) if inp is None else inp["mask"], dtype)
    if "g" in fl:
        kw["raw"] = out = full((M, prob.N), dtype)
    if "s" in fl:
        kw["stats"] = full((M // 64, prob.N, 2), torch.float32)
    if "w" in fl:
        kw["rowpart"] = full((M, prob.N // rowspan, 2), torch.float32)
    return pk, x, kw, out


def plan_of(ops, prob, dtype=torch.bfloat16, rowspan=0):
    pk, x, kw, _out = launch_args(ops, prob, dtype, rowspan=rowspan)
    return ops.conv_gemm_plan(x, pk, *prob.geom, **kw)
