// Private to the conv / GEMM translation units (conv_gemm.hip, conv_gemm2.hip, conv_halo.hip, gemm_pps.hip, gemm_ws.hip): the plan
// launch_conv_gemm acts on, the tile forms of the kernel families as tables, what each unit offers the planner, and the environment
// switches of the family.  The public launch interface is kernels.h.
#pragma once
#include <cstdlib>
#include "kernels.h"

// kind: what conv_gemm_kind reports
enum { KIND_GENERAL = 0, KIND_HALO = 1, KIND_HALO_PERSIST = 2, KIND_WS = 3, KIND_PPS = 4 };

// ---- tile forms ---------------------------------------------------------------------------------------------------------------
// conv_halo_kernel<TN, WN, MI> / conv_halo_persist_kernel<TN, WN>: 8 waves as (8 / WN) x WN, a wave owns 128 rows x TN * 16 columns.
// In the order conv_halo_plan prefers them (the halo-resident input is cheap, the streamed weights are not: 512-pixel tiles first).
struct HaloForm {
  int id, tn, wn;
  bool multi_image;  // at the 8 x 8 level a tile is four whole images and the chunks are split (conv_halo_kernel<.., true>); only so
  bool persist;      // has a conv_halo_persist_kernel instantiation (short K loops: the decoder's levels)
  constexpr int bm() const { return (8 / wn) * 128; }
  constexpr int bn() const { return wn * tn * 16; }
};
constexpr int HALO_NARROW = 1, HALO_512x128 = 2, HALO_256x256 = 4, HALO_256x320 = 5, HALO_512x160 = 6;     // the ids dd_op_conv_halo_plan reports
constexpr HaloForm HALO_FORMS[] = {
    {HALO_512x160, 5, 2, false, false},
    {HALO_512x128, 4, 2, false, true},    // (N % 160 != 0: the decoder)
    {HALO_256x320, 5, 4, true, false},
    {HALO_256x256, 4, 4, false, false},
    {HALO_NARROW, 1, 2, false, false},    // 512 x 32: conv_out (N <= 4), outside the preference order
};
constexpr HaloForm halo_form(int id) {
  for (const HaloForm& f : HALO_FORMS)
    if (f.id == id) return f;
  return HaloForm{0, 1, 2, false, false};
}
// A halo launch, decided once (conv_halo.hip: conv_halo_plan) and acted on as it stands (launch_conv_halo).  geo is what the kernels get:
// a tile is th x tw OUTPUT pixels of one image (th * tw = 256 or 512, tw = 1 << ltw a power of two >= 16 that divides Wo), tiles_x x
// tiles_y of them per image; its halo is halo_px = (th + 2) x (tw + 2) LOGICAL input pixels (the fused nearest-2x upsample reads stored
// pixel (iy >> shift, ix >> shift)); ipt = images per tile (4 at 8 x 8: a tile is 4 whole images, each with its own 10 x 10 halo block);
// tab = the kernel keeps a halo address table in LDS.
struct HaloGeo { int ltw, th, halo_px, tiles_x, tiles_y, ipt, tab; };
struct HaloPlan {
  int form, kind, split;       // HALO_FORMS id; KIND_HALO / KIND_HALO_PERSIST; chunk split of the 8 x 8 level (the kernel's p.ksplit), 1: none
  HaloGeo geo;
  int lds, grid_x, grid_y;     // dynamic LDS bytes; workgroups (grid_y = split)
};

// conv_gemm_big_kernel<WM, WN, TM, TN, NS, ...>: WM x WN waves of TM x TN MFMA tiles, NS LDS stages; index = the configuration that
// conv_gemm_big_config returns and dd_op_conv_gemm_plan reports (0: not the big kernel).  8 waves: one workgroup per CU; 4 waves: two
// (shallow K), and only those have the CF_ROWSTATS epilogue, one partial per wave span of TN * 16 columns.
struct BigForm {
  int wm, wn, tm, tn, ns, rowstat_span;
  constexpr int bm() const { return wm * tm * 16; }
  constexpr int bn() const { return wn * tn * 16; }
};
constexpr BigForm BIG_FORMS[6] = {
    {0, 0, 0, 0, 0, 0},
    {2, 4, 4, 4, 3, 0},        // 1: 128 x 256
    {4, 2, 4, 5, 3, 0},        // 2: 256 x 160
    {4, 2, 4, 4, 3, 0},        // 3: 256 x 128
    {2, 2, 4, 5, 2, 80},       // 4: 128 x 160, two workgroups per CU
    {2, 2, 4, 4, 2, 64},       // 5: 128 x 128, two workgroups per CU (GEGLU / N % 128 == 0)
};

// ---- the launcher's decision (conv_gemm.hip: plan_problem) ------------------------------------------------------------------------
struct ConvPlan {
  int kind;          // KIND_*
  int form;          // the form inside the kind: general = conv_gemm_big_kernel configuration (BIG_FORMS; 0 = conv_gemm_kernel), halo = HALO_FORMS id,
                     // ws / pps = TN (5: 320-column blocks, 4: 256-column GEGLU blocks)
  int split;         // split-K of the general kernels / chunk split of the halo 8 x 8 form; > 1: splitk_reduce_kernel follows
  int narrow;        // conv_gemm_kernel runs its 256 x 64 tiles instead of 128 x 128
  bool empty;        // M <= 0 or N <= 0: accepted, nothing to launch
  bool stats;        // CF_STATS is honoured
  int row_spans;     // CF_ROWSTATS is honoured with this many (sum, sum^2) pairs per row; 0: not asked
  HaloPlan halo;     // kind KIND_HALO / KIND_HALO_PERSIST: the whole launch
};

// ---- what the units offer the planner: *_config return 0 (not eligible: shape, flags, alignment, 32-bit offsets) or the form ----------
int conv_gemm_big_config(int M, int N, int K, int flags);                        // conv_gemm2.hip
hipError_t launch_conv_gemm_big(const ConvGemmParams& p, int cfg, hipStream_t stream);
bool conv_halo_plan(const ConvGemmParams& p, size_t partial_cap_bytes, HaloPlan* hp);   // conv_halo.hip: deep 3x3 / stride 1, halo-resident input
hipError_t launch_conv_halo(const ConvGemmParams& p, const HaloPlan& hp, hipStream_t stream);
int gemm_ws_config(const ConvGemmParams& p);                                     // gemm_ws.hip: weight-stationary GEMM (K = 320 pointwise layers)
int gemm_ws_rowstat_spans(const ConvGemmParams& p);
hipError_t launch_gemm_ws(const ConvGemmParams& p, int tn, hipStream_t stream);
int gemm_pp_config(const ConvGemmParams& p);                                     // gemm_pps.hip: persistent pointwise ping-pong GEMM
int gemm_pp_rowstat_spans(const ConvGemmParams& p);
hipError_t launch_gemm_pp(const ConvGemmParams& p, int tn, hipStream_t stream);

// ---- environment switches of the family, read once per process on first use ------------------------------------------
struct ConvEnv {
  int conv_halo, halo_tall, halo_8x8, halo_narrow, halo_persist, halo_tab;       // DD_CONV_HALO, DD_HALO_TALL, DD_HALO_8X8, DD_HALO_NARROW, DD_HALO_PERSIST, DD_HALO_TAB
  int gemm_ws, gemm_ws_mask;                                                     // DD_GEMM_WS, DD_GEMM_WS_MASK (1 GEGLU, 2 row statistics, 4 LayerNorm-folded, 8 the rest)
  int gemm_pp, gemm_pp_geglu;                                                    // DD_GEMM_PP, DD_GEMM_PP_GEGLU
};
inline const ConvEnv& conv_env() {
  static const ConvEnv e = [] {
    auto get = [](const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; };
    return ConvEnv{get("DD_CONV_HALO", 1), get("DD_HALO_TALL", 1), get("DD_HALO_8X8", 1), get("DD_HALO_NARROW", 1), get("DD_HALO_PERSIST", 1),
                   get("DD_HALO_TAB", 1), get("DD_GEMM_WS", 1), get("DD_GEMM_WS_MASK", 15), get("DD_GEMM_PP", 1), get("DD_GEMM_PP_GEGLU", 1)};
  }();
  return e;
}
