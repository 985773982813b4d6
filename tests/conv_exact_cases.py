"""The case table of the exact-input tests of the conv / GEMM kernels, and the one function that turns a case into the arguments of
ops.conv_gemm / ops.conv_gemm_plan.  No device is needed to import this or to ask the planner (tests/test_conv_exact_cases.py walks the
table on the CPU); tests/test_conv_exact_gpu.py runs it.

A case is (Problem, plan, f16): the problem in the terms of tests/exact_ref.py, the (kind, form, split) the launcher must give it, and
whether the fp16 library runs it too (one case per kind and form).  The shapes are the smallest the planner routes as stated; tuples in
the comments are (B, Cin, Cout, H, W).  Halo kinds need M >= 49152 rows.

STAT_CASES is the second table: the statistics epilogues, the LayerNorm fold and the GEGLU product, which have closed forms on the
ternary family only (exact_ref.expected_buffers); STAT_REFUSALS is what the launcher must refuse of them.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_conv_big_bits as big  # noqa: E402
import make_pingpong_bits as pp  # noqa: E402
import exact_ref as X  # noqa: E402
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
    # 4 image rows of 128 pixels: 256 x 320 tiles at tw = 128, th = 2, whose halo address table does not fit the LDS (166 464 B): the
    # per-piece address arithmetic of the one-tile kernel, reached without DD_HALO_TAB=0 (tests/golden/halo_plan_table.npz: table = 0)
    conv("halo_4x128_table_does_not_fit", 48, 64, 640, 4, 128, (HALO, None, 1), f16=True),
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


# ---- the statistics epilogues (CF_STATS "s", CF_ROWSTATS "w"), the LayerNorm fold ("l") and the GEGLU product ("G", "g"): ternary only ----
# A case is (Problem, plan, f16, rowspan, slots): rowspan is the span layout of a "w" case (span_list), slots names the CF_STATS slot map
# of an "s" case ("m64": m >> 6; "halo": exact_ref.slots_halo).  One case per (kernel or form) x (flag set) the launcher honours.  No
# kernel honours "l" together with "w" (rowstats_shape_ok refuses CF_LNFOLD) or "s" together with "w"; both are asserted as refusals in
# tests/test_conv_exact_cases.py.

def sconv(name, B, Cin, Cout, H, W, plan, fl, f16=False, slots="m64", **kw):
    kw.setdefault("ksplit", 1 if plan[0] == G else 0)
    return Problem(name, B, Cin, Cout, H, W, fl=fl, **kw), plan, f16, 0, slots


def sgemm(name, M, K, N, plan, fl, f16=False, rowspan=0, ksplit=1):
    return Problem(name, 1, K, N, M, 1, k=1, fl=fl, ksplit=ksplit), plan, f16, rowspan, "m64"


STAT_CASES = [
    # ---- CF_STATS on conv_gemm_big_kernel: FE epilogue of every form ----
    sconv("s_big_128x256", 2, 512, 256, 24, 24, (G, F1, 1), "bs", f16=True),
    sconv("s_big_128x256_res_relu", 2, 512, 256, 24, 24, (G, F1, 1), "brus"),
    sconv("s_big_256x160", 2, 1280, 320, 24, 24, (G, F2, 1), "bs", f16=True),
    sconv("s_big_256x128", 2, 512, 128, 32, 32, (G, F3, 1), "bs", f16=True),
    sconv("s_big_128x160_two_workgroups_res", 2, 320, 320, 24, 24, (G, F4, 1), "brs", f16=True),
    sconv("s_big_128x160_two_workgroups_pointwise_res", 4, 1280, 320, 32, 32, (G, F4, 1), "brs", k=1),
    sconv("s_big_128x128_two_workgroups_res", 3, 128, 384, 32, 32, (G, F5, 1), "brs", f16=True),
    # ---- CF_STATS on the halo kernels: slot m >> 6, and the block map of tiles narrower than 64 pixels ----
    sconv("s_halo_320_32x32_res", 48, 320, 320, 32, 32, (HALO, None, 1), "brs", f16=True),
    sconv("s_halo_320_32x32_res_relu", 48, 320, 320, 32, 32, (HALO, None, 1), "brus"),
    sconv("s_halo_640_16x16", 192, 128, 640, 16, 16, (HALO, None, 1), "bs"),
    sconv("s_halo_up2_320", 24, 128, 320, 32, 32, (HALO, None, 1), "bs", up=1),
    sconv("s_halo_w48_block_map", 24, 64, 320, 48, 48, (HALO, None, 1), "bs", f16=True, slots="halo"),
    sconv("s_halo_w80_block_map", 8, 128, 320, 80, 80, (HALO, None, 1), "bs", slots="halo"),
    sconv("s_halo_w96_block_map_res", 6, 320, 320, 96, 96, (HALO, None, 1), "brs", slots="halo"),
    sconv("s_halo_4x128_table_does_not_fit_res", 48, 64, 640, 4, 128, (HALO, None, 1), "brs"),
    sconv("s_persist_256_64x64_res", 12, 64, 256, 64, 64, (PERSIST, None, 1), "brs", f16=True, slots="halo"),
    sconv("s_persist_w256_res", 1, 64, 256, 256, 256, (PERSIST, None, 1), "brs", slots="halo"),
    sconv("s_persist_n128_256x512_res", 1, 128, 128, 256, 512, (PERSIST, None, 1), "brs", slots="halo"),
    # ---- gemm_pps: CF_STATS, CF_ROWSTATS (80-column spans) ----
    sgemm("s_pps_n320_res", 49152, 320, 320, (PPS, None, 1), "brs", f16=True),
    sgemm("s_pps_n320_res_relu", 49152, 320, 320, (PPS, None, 1), "brus"),
    sgemm("w_pps_n320_res", 49152, 320, 320, (PPS, None, 1), "brw", f16=True, rowspan=80),
    sgemm("w_pps_n640_k1280_res", 49152, 1280, 640, (PPS, None, 1), "brw", rowspan=80),
    # ---- gemm_ws: CF_ROWSTATS in 48 + 32 column spans ----
    sgemm("w_ws_n320", 33024, 320, 320, (WS, None, 1), "bw", f16=True, rowspan="ws"),
    sgemm("w_ws_n640_relu", 36928, 320, 640, (WS, None, 1), "buw", rowspan="ws"),
    sgemm("w_ws_n640_views", 32768, 320, 640, (WS, None, 1), "bwv", rowspan="ws"),
    # ---- CF_ROWSTATS on the two-workgroup forms of conv_gemm_big_kernel ----
    sgemm("w_big_128x160_two_workgroups_res", 2048, 320, 320, (G, F4, 1), "brw", f16=True, rowspan=80),
    sgemm("w_big_128x160_two_workgroups_res_ragged_m", 3000, 640, 1280, (G, F4, 1), "brw", rowspan=80),
    sgemm("w_big_128x128_two_workgroups_res", 4096, 320, 384, (G, F5, 1), "brw", f16=True, rowspan=64),
    # ---- CF_LNFOLD: the generic epilogue of the small kernel, the folded epilogue of the two-workgroup forms, gemm_ws, gemm_pps ----
    sgemm("l_small_256x64", 300, 320, 320, (G, S256, 1), "bl", f16=True),
    sgemm("l_small_128x128", 64, 320, 320, (G, S128, 1), "bl", f16=True),
    sgemm("l_small_256x64_alpha", 300, 320, 320, (G, S256, 1), "bla"),
    sgemm("l_big_128x160_two_workgroups", 2048, 640, 640, (G, F4, 1), "bl", f16=True),
    sgemm("l_big_128x160_two_workgroups_alpha", 2048, 640, 640, (G, F4, 1), "bla"),
    sgemm("l_big_128x160_two_workgroups_n3840", 1024, 1280, 3840, (G, F4, 1), "bl"),
    sgemm("l_ws_n960", 33088, 320, 960, (WS, None, 1), "bl", f16=True),
    sgemm("l_ws_n960_alpha", 33088, 320, 960, (WS, None, 1), "bla"),
    sgemm("l_pps_n640", 49152, 640, 640, (PPS, None, 1), "bl", f16=True),
    sgemm("l_pps_n640_alpha", 49152, 640, 640, (PPS, None, 1), "bla"),
    # ---- GEGLU: y = hidden * gelu_poly(gate), with the fold and with the raw stash ----
    sgemm("G_big_128x128_two_workgroups_fold", 1024, 320, 2560, (G, F5, 1), "bGl", f16=True),
    sgemm("G_big_128x128_two_workgroups_fold_alpha", 1024, 320, 2560, (G, F5, 1), "bGla"),
    sgemm("g_big_128x128_two_workgroups_fold_raw", 1024, 320, 512, (G, F5, 1), "bgl"),
    sgemm("G_big_128x128_two_workgroups_ragged_m", 1500, 320, 2560, (G, F5, 1), "bG", f16=True),
    sgemm("G_small_128x128", 200, 128, 512, (G, S128, 1), "bG", f16=True),
    sgemm("g_ws_n2560_fold_raw", 33088, 320, 2560, (WS, None, 1), "bgl", f16=True),
    sgemm("G_ws_n512", 32832, 320, 512, (WS, None, 1), "bG", f16=True),
    sgemm("G_pps_n1024_fold", 12288, 320, 1024, (PPS, None, 1), "bGl", f16=True),
    sgemm("G_pps_n2560_k640_fold", 24576, 640, 2560, (PPS, None, 1), "bGl"),
    sgemm("G_pps_n1024_fold_alpha", 12288, 320, 1024, (PPS, None, 1), "bGla"),
    sgemm("g_pps_raw_stash_and_y", 40960, 256, 512, (PPS, None, 1), "bg", f16=True),
    # ---- the fold and GEGLU on every other recorded (form, split): the generic epilogue (Epi::apply) of the eight-wave forms and of the
    # small kernel, and the split-K reduce kernel (the smallest GEMMs the planner routes so; ksplit = 4 is the caller's) ----
    sgemm("G_small_128x128_fold", 64, 128, 64, (G, S128, 1), "bGl", ksplit=0),
    sgemm("G_small_128x128_splitk2", 64, 128, 64, (G, S128, 2), "bG", ksplit=4),
    sgemm("l_small_128x128_splitk2", 64, 128, 64, (G, S128, 2), "bl", ksplit=4),
    sgemm("G_small_128x128_splitk2_fold", 64, 128, 64, (G, S128, 2), "bGl", ksplit=4),
    sgemm("G_small_256x64", 256, 128, 64, (G, S256, 1), "bG", f16=True, ksplit=0),
    sgemm("G_small_256x64_fold", 256, 128, 64, (G, S256, 1), "bGl", ksplit=0),
    sgemm("G_small_256x64_splitk2", 256, 128, 64, (G, S256, 2), "bG", ksplit=4),
    sgemm("l_small_256x64_splitk2", 256, 128, 64, (G, S256, 2), "bl", ksplit=4),
    sgemm("G_small_256x64_splitk2_fold", 256, 128, 64, (G, S256, 2), "bGl", ksplit=4),
    sgemm("G_big_128x256", 1024, 2560, 256, (G, F1, 1), "bG", f16=True),
    sgemm("l_big_128x256", 1024, 2560, 256, (G, F1, 1), "bl", f16=True),
    sgemm("G_big_128x256_fold", 1024, 2560, 256, (G, F1, 1), "bGl"),
    sgemm("G_big_128x256_splitk4", 1024, 2560, 256, (G, F1, 4), "bG", ksplit=4),
    sgemm("l_big_128x256_splitk4", 1024, 2560, 256, (G, F1, 4), "bl", ksplit=4),
    sgemm("G_big_128x256_splitk4_fold", 1024, 2560, 256, (G, F1, 4), "bGl", ksplit=4),
    sgemm("G_big_256x128", 1024, 128, 64, (G, F3, 1), "bG", f16=True),
    sgemm("l_big_256x128", 1024, 128, 64, (G, F3, 1), "bl", f16=True),
    sgemm("G_big_256x128_fold", 1024, 128, 64, (G, F3, 1), "bGl"),
    sgemm("G_big_256x128_splitk2", 1024, 128, 64, (G, F3, 2), "bG", ksplit=4),
    sgemm("l_big_256x128_splitk2", 1024, 128, 64, (G, F3, 2), "bl", ksplit=4),
    sgemm("G_big_256x128_splitk2_fold", 1024, 128, 64, (G, F3, 2), "bGl", ksplit=4),
    sgemm("l_big_128x160_two_workgroups_splitk2", 1024, 128, 320, (G, F4, 2), "bl", ksplit=4),
    sgemm("l_big_128x128_two_workgroups", 1024, 128, 128, (G, F5, 1), "bl", f16=True),
    sgemm("G_big_128x128_two_workgroups_splitk2", 1024, 128, 128, (G, F5, 2), "bG", ksplit=4),
    sgemm("l_big_128x128_two_workgroups_splitk2", 1024, 128, 128, (G, F5, 2), "bl", ksplit=4),
    sgemm("G_big_128x128_two_workgroups_splitk2_fold", 1024, 128, 128, (G, F5, 2), "bGl", ksplit=4),
]
STAT_NAMES = [c[0].name for c in STAT_CASES]


def stat_expected(prob, acc, inp, dtype, rowspan, slots, mutant=None, check=True):
    """exact_ref.expected_buffers for a case of STAT_CASES (or one cut to fewer rows), with the exactness conditions asserted first;
    returns (buffers, bounds found)"""
    spans = span_list(prob, rowspan) if "w" in prob.fl else None
    slot_of = (X.slots_halo if slots == "halo" else X.slots_m64)(prob) if "s" in prob.fl else None
    bufs = X.expected_buffers(prob, acc, inp, dtype, spans, slot_of, mutant)
    found = None
    if check:
        assert mutant is None
        X.check_conditions(prob, inp, "ternary", dtype, ref=None if "l" in prob.fl or "g" in prob.fl or "G" in prob.fl else bufs["y"])
        found = X.check_stat_conditions(prob, inp, bufs, dtype, spans, slot_of)
    return bufs, found

# what the launcher refuses: (Problem, rowspan) -- asserted as refusals on the CPU, never run
STAT_REFUSALS = [
    (Problem("s_ragged_m", 2, 320, 320, 24, 25, fl="bs", ksplit=1), 0),                      # CF_STATS needs whole 64-row blocks
    (Problem("s_small_kernel", 2, 64, 128, 16, 16, fl="bs"), 0),                             # the small kernel has no CF_STATS epilogue
    (Problem("s_halo_8x8", 32, 2560, 1280, 8, 8, fl="bs"), 0),                               # nor has the chunk-split form of the 8 x 8 level
    (Problem("s_and_w_pps", 1, 1280, 640, 49152, 1, k=1, fl="bsw", ksplit=1), 80),           # one statistics epilogue per launch
    (Problem("w_m512_too_few_work_items", 1, 320, 320, 512, 1, k=1, fl="brw", ksplit=1), 80),
    (Problem("l_and_w_ws", 1, 320, 320, 33024, 1, k=1, fl="blw", ksplit=1), "ws"),           # no kernel honours the fold with row partials
    (Problem("l_and_w_big", 1, 320, 320, 2048, 1, k=1, fl="blw", ksplit=1), 80),
    (Problem("l_and_w_pps", 1, 320, 320, 49152, 1, k=1, fl="blw", ksplit=1), 80),
]


def record_problems():
    """{"big:case" | "pp:case": (Problem, salt, rowstat span | 0, plan | kind index)} for every case of the two bit records, in the flag
    letters of exact_ref (G: GEGLU without the stash, l: CF_LNFOLD -- on the records' lattice inputs neither has a closed form for y)"""
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
    """the outputs of a case that exact_ref derives on LATTICE inputs (the bit records): "raw" for the stash, "y" unless GELU or the
    LayerNorm fold is in it (STAT_CASES derives every output, on ternary inputs)"""
    if "g" in prob.fl:
        return ["raw"]
    return [] if ("G" in prob.fl or "l" in prob.fl) else ["y"]


def span_list(prob, rowspan):
    """the column spans of a CF_ROWSTATS case: a list of widths as it is, one width for the whole row, "ws" for gemm_ws's 48 + 32"""
    if rowspan == "ws":
        return [48, 32] * (prob.N // 80)
    return list(rowspan) if isinstance(rowspan, (list, tuple)) else [rowspan] * (prob.N // rowspan)


def launch_args(ops, prob, dtype=torch.bfloat16, inp=None, dev="cpu", rowspan=0, bufs=None):
    """(pk, x, kw, out): the packed weights, the input rows and the keywords of ops.conv_gemm / ops.conv_gemm_plan for one case, and
    `out`, the WHOLE buffer that is compared (the output with its NaN-prefilled spare columns; the raw stash for "g").  inp = None (the
    planner: it only tests pointers for null): buffers of the right shape that nobody reads.  bufs: a dict that receives EVERY whole
    buffer of the launch under the names of exact_ref.expected_buffers ("y", "raw", "stats", "rowpart"): the statistics go into views of
    NaN-prefilled wider buffers (partials: channels [64, 64 + N) of [M / 64, 64 + N, 2]; row partials: the first spans of
    [M, spans + 3, 2])."""
    fl = prob.fl
    bufs = {} if bufs is None else bufs
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
    bufs["y"] = ybuf
    if "g" in fl:
        kw["raw"] = out = bufs["raw"] = full((M, prob.N), dtype)
    if "s" in fl:
        bufs["stats"] = full((M // 64, X.STATS_PAD + prob.N, 2), torch.float32)
        kw["stats"] = bufs["stats"][:, X.STATS_PAD:]
    if "w" in fl:
        nspans = len(span_list(prob, rowspan))
        bufs["rowpart"] = full((M, nspans + X.SPAN_PAD, 2), torch.float32)
        kw["rowpart"] = bufs["rowpart"][:, :nspans]
    if "l" in fl:
        # the synthetic (mean, rstd) rows and c1 in the packed column order (a second PackedConv: it reuses the bias permutation)
        kw["ln_stats"] = put((M, 2) if inp is None else inp["ln_stats"], torch.float32)
        c1 = torch.zeros(prob.N) if inp is None else X.ln_c1(inp)
        kw["ln_c1"] = ops.PackedConv(w, prob.pad, geglu="g" in fl or "G" in fl, bias=c1, device=dev, dtype=dtype).bias
    return pk, x, kw, out


def plan_of(ops, prob, dtype=torch.bfloat16, rowspan=0):
    pk, x, kw, _out = launch_args(ops, prob, dtype, rowspan=rowspan)
    return ops.conv_gemm_plan(x, pk, *prob.geom, **kw)
