"""The exact-input cases of the attention kernels (tests/attention_exact_ref.py has the families and the closed form): small shapes at
the tile edges, each with the plan it is about.  tests/test_attention_exact_cases.py walks the table on the CPU (plans, exactness
conditions, coverage of the engine's plans, mutants), tests/test_attention_exact_gpu.py runs it.

Key counts 1, 13, 16, 64, 65, 77, 80, 81 (the first past the short-key kernel), 130, 200, 1064 and 4096 (ring wrap-around of the LDS-DMA
kernel); ragged (50, 77, 200, 300) and full query counts; one, four and eight 32-query tiles per short-key wave; head dims 32, 40, 64,
80, 160, 256, 512; causal, q_prescaled, pv_fp8, no_shortk, q / k / v as column views of a fused projection; the GEMM route with scratch
for 1, 2 and 8 images (5 images in groups of 2); f16: the case also runs on the fp16 storage build (once per route).

| route                      | family                  | why                                                                                        |
| short-key, LDS-DMA lazy    | graded (and one mask)   | log2-domain kernels: integer scores, power-of-two probabilities                            |
| fp8 P.V                    | graded, depth 5, v <= 4 | e4m3 holds every p in 2^-5 .. 2^5 and every v                                              |
| LDS-DMA non-lazy, register | mask at 1 / sqrt(D),    | the kernels scale the scores themselves: fp32 ln 2 * log2 e is exactly 1, any other scale  |
| staged (d = 160, 512,      | graded at ln 2          | needs probabilities of exactly 1 or 0                                                      |
| causal)                    |                         |                                                                                            |
| GEMM route, forward        | mask at 1 / sqrt(D),    | softmax_rows_kernel rounds p / l to the stored format in front of the P.V GEMM             |
|                            | 2^m visible keys        |                                                                                            |
| flash backward             | graded at ln 2, l = 2^m | plain and PS, ragged last tile, need_dkv off                                               |
| GEMM route, backward       | mask at 2^-4, D = 256   | the route scales dS in front of its rounding: a power-of-two scale keeps the bits unique;  |
|                            |                         | at the model's 1 / sqrt(512) the route is covered FORWARD ONLY                             |
"""
import ctypes as C

import torch

from attention_exact_ref import Case


def P(route, d=0, qt=0, kt=0, dsplit=0, ktw=0, qtl=0, waves=0, lazy=False, prescaled=False, causal=False, fp8=False, **more):
    return dict(route=route, d=d, qt=qt, kt=kt, dsplit=dsplit, ktw=ktw, qtl=qtl, waves=waves, lazy=lazy, prescaled=prescaled, causal=causal,
                fp8=fp8, **more)


def SK(d, waves, **more):
    return P("shortk", d=d, waves=waves, **more)


def DMA(d, waves, lazy, **more):
    return P("dma", d=d, qt=2, kt=64, dsplit=1, waves=waves, lazy=lazy, **more)


FP8 = P("dma", d=64, qt=2, kt=128, dsplit=1, waves=8, lazy=True, fp8=True)


def STREAM(d, **more):
    return P("stream", d=d, qt=4 if d == 512 else 2, kt=32 if d == 512 else 64, dsplit=4 if d == 512 else 1, waves=4, **more)


def BWD(d, ps, dkv=True):
    qt = 2 if d <= 64 else 1
    return P("flash_bwd", d=d, qt=qt, kt=32 if d == 512 else 64, dsplit=4 if d == 512 else 1, ktw=qt if dkv else 0,
             qtl=(32 if d == 512 else 64) if dkv else 0, waves=4, prescaled=ps)


def GEMM(group):
    return P("gemm", group=group)


CASES = [
    # ---- the short-key kernel (<= 80 keys, whole 32-query tiles): its score tiles are 16 keys.  The first case decides whether the
    # hardware exp2 returns exact powers of two for integral arguments
    Case("sk_d40_pre_k77", 2, 3, 256, 77, 40, SK(40, 8, grid=24), prescaled=True, kt=16, f16=True),
    Case("sk_d64_pre_k1", 1, 2, 64, 1, 64, SK(64, 4), prescaled=True, kt=16),
    Case("sk_d80_k13", 2, 2, 96, 13, 80, SK(80, 4), kt=16),
    Case("sk_d40_k16", 1, 2, 32, 16, 40, SK(40, 8), kt=16),
    Case("sk_d64_pre_k64", 1, 3, 128, 64, 64, SK(64, 4), prescaled=True, kt=16),
    Case("sk_d80_pre_k65", 1, 2, 160, 65, 80, SK(80, 4), prescaled=True, kt=16),
    Case("sk_d40_k80", 2, 2, 512, 80, 40, SK(40, 8), kt=16),
    Case("sk_d40_mask_k77", 1, 4, 64, 77, 40, SK(40, 8), family="mask", kt=16),
    Case("sk_d64_pre_k77_4_tiles_per_wave", 64, 16, 512, 77, 64, SK(64, 4, grid=1024), prescaled=True, kt=16),
    Case("sk_d64_pre_k77_8_tiles_per_wave", 64, 16, 1024, 77, 64, SK(64, 4, grid=1024), prescaled=True, kt=16),
    # ---- LDS-DMA kernel, lazy-reference softmax (prescaled query)
    Case("dma_d40_w8_pre_k81", 1, 2, 256, 81, 40, DMA(40, 8, True), prescaled=True),
    Case("dma_d40_w4_pre_q300_k130", 2, 2, 300, 130, 40, DMA(40, 4, True), prescaled=True, f16=True),
    Case("dma_d40_w8_pre_q512_k4096_ring", 1, 2, 512, 4096, 40, DMA(40, 8, True), prescaled=True),
    Case("dma_d64_pre_q200_k200_wide", 2, 2, 200, 200, 64, DMA(64, 4, True), prescaled=True, wide=True),
    Case("dma_d64_pre_k200_optimistic_sweep_suffices", 1, 2, 256, 200, 64, DMA(64, 4, True), prescaled=True, late=False),
    Case("dma_d80_pre_q77_k1064_needs_safe_sweep", 1, 3, 77, 1064, 80, DMA(80, 4, True), prescaled=True),
    Case("dma_d32_pre_q50_k65", 2, 2, 50, 65, 32, DMA(32, 4, True), prescaled=True),
    Case("dma_d40_pre_k77_no_shortk", 1, 2, 256, 77, 40, DMA(40, 8, True), prescaled=True, no_shortk=True),
    # ---- fp8 P.V (d = 64, 128-key tiles, always the safe sweep)
    Case("fp8_d64_pre_q256_k200", 1, 2, 256, 200, 64, FP8, prescaled=True, fp8=True, kt=128),
    Case("fp8_d64_q300_k1064", 1, 2, 300, 1064, 64, FP8, fp8=True, kt=128),
    Case("fp8_d64_pre_q64_k77", 1, 2, 64, 77, 64, FP8, prescaled=True, fp8=True, kt=128),
    # ---- LDS-DMA kernel, online softmax (the kernel scales the scores)
    Case("dma_d40_w8_ln2_q256_k200", 1, 2, 256, 200, 40, DMA(40, 8, False)),
    Case("dma_d64_mask_q50_k50_wide", 2, 3, 50, 50, 64, DMA(64, 4, False), family="mask", wide=True, f16=True),
    Case("dma_d40_w8_mask_q256_k1064", 1, 2, 256, 1064, 40, DMA(40, 8, False), family="mask"),
    Case("dma_d80_mask_q200_k81", 1, 2, 200, 81, 80, DMA(80, 4, False), family="mask"),
    Case("dma_d32_ln2_q96_k130", 1, 2, 96, 130, 32, DMA(32, 4, False)),
    # ---- register-staged kernel: d = 160, d = 512 without scratch (head dim split over the waves, 32-key tiles), causal
    Case("stream_d160_mask_q77_k77", 2, 2, 77, 77, 160, STREAM(160), family="mask", f16=True),
    Case("stream_d160_mask_q64_k200", 1, 2, 64, 200, 160, STREAM(160), family="mask"),
    Case("stream_d160_pre_q64_k130", 1, 2, 64, 130, 160, STREAM(160), prescaled=True),
    Case("stream_d512_mask_q200_k130", 1, 1, 200, 130, 512, STREAM(512), family="mask", kt=32, f16=True),
    Case("stream_d512_ln2_q64_k65", 2, 1, 64, 65, 512, STREAM(512), kt=32),
    Case("causal_d64_mask_77", 3, 2, 77, 77, 64, STREAM(64, causal=True), family="mask", causal=True),
    Case("causal_d64_mask_130", 2, 2, 130, 130, 64, STREAM(64, causal=True), family="mask", causal=True),
    Case("causal_d40_ln2_130", 1, 2, 130, 130, 40, STREAM(40, causal=True), causal=True),
    # ---- GEMM route, forward only at the model's 1 / sqrt(D).  ops.attention_gemm sizes its scratch for the backward, 2.57 forward
    # images per image at 256 x 256 x 512: scratch "for one image" runs the forward's five images in groups of two
    Case("gemm_d512_ws1_groups_2_2_1", 5, 1, 256, 256, 512, GEMM(2), api="gemm", family="mask", ws_images=1, f16=True),
    Case("gemm_d512_ws2_one_group_of_5", 5, 1, 256, 256, 512, GEMM(5), api="gemm", family="mask", ws_images=2),
    Case("gemm_d512_ws8_groups_8_1", 9, 1, 256, 256, 512, GEMM(8), api="gemm", family="mask", ws_images=8),
    Case("gemm_d256_two_heads_q128_k192", 2, 2, 128, 192, 256, GEMM(1), api="gemm", family="mask", ws_images=8),
    Case("gemm_d512_planned_entry", 2, 1, 256, 256, 512, GEMM(2), api="planned", family="mask", ws_images=2),
    # ---- backward: dQ, dK, dV bit for bit
    Case("bwd_d40_ps_q128_k130", 2, 2, 128, 130, 40, DMA(40, 4, True), BWD(40, True), prescaled=True, f16=True),
    Case("bwd_d40_ps_cross_q64_k77", 1, 2, 64, 77, 40, SK(40, 8), BWD(40, True, False), prescaled=True, need_dkv=False),
    Case("bwd_d64_q200_k200", 1, 2, 200, 200, 64, DMA(64, 4, False), BWD(64, False)),
    Case("bwd_d64_ps_q130_k130_wide", 1, 2, 130, 130, 64, DMA(64, 4, True), BWD(64, True), prescaled=True, wide=True),
    Case("bwd_d64_ps_cross_q96_k77", 1, 2, 96, 77, 64, SK(64, 4), BWD(64, True, False), prescaled=True, need_dkv=False),
    Case("bwd_d80_ps_q77_k200", 1, 2, 77, 200, 80, DMA(80, 4, True), BWD(80, True), prescaled=True),
    Case("bwd_d80_ps_cross_q256_k77", 1, 2, 256, 77, 80, SK(80, 4), BWD(80, True, False), prescaled=True, need_dkv=False),
    Case("bwd_d160_ps_q64_k64", 2, 2, 64, 64, 160, STREAM(160), BWD(160, True), prescaled=True),
    Case("bwd_d160_ps_cross_q64_k77", 1, 2, 64, 77, 160, STREAM(160), BWD(160, True, False), prescaled=True, need_dkv=False),
    Case("bwd_d512_q50_k81", 1, 1, 50, 81, 512, STREAM(512), BWD(512, False), kt=32),
    Case("bwd_d32_q96_k65", 1, 2, 96, 65, 32, DMA(32, 4, False), BWD(32, False)),
    Case("bwd_gemm_d256_two_heads_q128_k192", 2, 2, 128, 192, 256, GEMM(1), GEMM(1), api="gemm", family="mask", scale=2.0 ** -4, ws_images=8, f16=True),
    Case("bwd_gemm_d256_groups_2_1", 3, 1, 256, 256, 256, GEMM(3), GEMM(2), api="gemm", family="mask", scale=2.0 ** -4, ws_images=2),
]
NAMES = [c.name for c in CASES]

_NOT_READ = 1 << 12       # stands for a buffer: the planner tests pointers for null and never follows them
O_PAD = 8                 # the kernels' o is columns O_PAD .. O_PAD + H D of a NaN-prefilled buffer O_PAD columns wider on either side


def scratch_bytes(ops, case, bwd, dtype=torch.bfloat16):
    """the scratch the ops wrappers offer: sized for the backward (ops._attn_scratch), at least one image for ops.attention_gemm"""
    L = ops._L(dtype)
    L.dd_op_attention_gemm_workspace.restype = C.c_size_t
    n = max(1, case.ws_images) if case.api == "gemm" else case.ws_images
    return L.dd_op_attention_gemm_workspace(case.Nq, case.Nk, case.D, 1) * n


def plan_of(ops, case, bwd=False, dtype=torch.bfloat16):
    """ops._attention_plan (dd_op_attention_plan) of the launch the GPU test makes for the case; no device is read"""
    from distdiff_amd._lib import AttnParams
    p = AttnParams()
    c = case.H * case.D
    p.q = p.k = p.v = p.o = p.lse = _NOT_READ
    p.ldq = p.ldk = p.ldv = 3 * c if case.wide else c
    p.ldo = c + 2 * O_PAD
    p.B, p.H, p.Nq, p.Nk, p.D, p.scale = case.B, case.H, case.Nq, case.Nk, case.D, case.scale
    p.causal, p.q_prescaled, p.pv_fp8, p.no_shortk = int(case.causal), int(case.prescaled), int(case.fp8), int(case.no_shortk)
    if bwd:
        p.d_o = p.dq = p.delta = _NOT_READ
        p.lddo = p.lddq = c
        if case.need_dkv:
            p.dk = p.dv = _NOT_READ
            p.lddk = p.lddv = c
    return ops._attention_plan(p, scratch_bytes(ops, case, bwd, dtype), bwd, dtype)


def plan_differences(got, want):
    """the fields of `want` (a P(...) dict; "grid": the first launch's grid.x) that `got` (ops._attention_plan) answers differently"""
    view = dict(got, grid=got["launches"][0][0] if got["launches"] else 0)
    return {k: (view[k], v) for k, v in want.items() if view[k] != v}


def plan_tuple(plan):
    """(route, d, qt, kt, dsplit, ktw, qtl, waves, bits) as tests/attention_plan_cases.py records them"""
    import attention_plan_cases as A
    bits = (A.BIT_LAZY if plan["lazy"] else 0) | (A.BIT_PRESCALED if plan["prescaled"] else 0) | (A.BIT_CAUSAL if plan["causal"] else 0) | (A.BIT_FP8 if plan["fp8"] else 0)
    return (A.ROUTES.index(plan["route"]), plan["d"], plan["qt"], plan["kt"], plan["dsplit"], plan["ktw"], plan["qtl"], plan["waves"], bits)
