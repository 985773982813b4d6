// Private to the attention translation units (attention.hip, attention_shortk.hip, attention_gemm.hip): the plan launch_attention acts on,
// the per-head-dim tile forms as one table, what each unit offers the launcher, and the environment switch of the family.  The public
// launch interface is kernels.h.
#pragma once
#include <cstdlib>
#include <type_traits>
#include "kernels.h"

// ---- the launcher's decision (attention.hip: attention_plan) ----------------------------------------------------------------------
// route: what attention_plan_query reports.  Forward: GEMM, SHORTK, DMA (attn_fwd_dma_kernel), STREAM (attn_fwd_kernel, register-staged);
// backward: GEMM or FLASH_BWD (attn_delta_kernel, attn_bwd_dq_kernel, and attn_bwd_dkv_kernel when dk / dv are asked for)
enum { ATTN_REFUSED = -1, ATTN_GEMM = 0, ATTN_SHORTK = 1, ATTN_DMA = 2, ATTN_STREAM = 3, ATTN_FLASH_BWD = 4 };
constexpr int ATTN_ANY = -2;                                   // attention_plan's `force`: no route asked for
struct AttnLaunch { dim3 grid; unsigned block; size_t lds; };
struct AttnPlan {
  int route = ATTN_REFUSED;
  int form = -1;       // row of ATTN_FORMS (the flash routes)
  int waves = 0;       // per workgroup
  bool lazy = false, prescaled = false, causal = false, fp8 = false;   // template flags of the kernels: lazy-reference softmax (DMA), the PS
                                                                       // instantiations of the backward, the causal mask (STREAM), fp8 P.V (DMA)
  int group = 0;       // GEMM: images per launch
  int sk_tiles = 0, sk_wgs = 0;   // SHORTK: 32-query tiles per (image, head), workgroups per (image, head)
  int launches = 0;    // of the flash routes, in order (FLASH_BWD: delta, dQ, dK/dV)
  AttnLaunch launch[3];
};
AttnPlan attention_plan(const AttnParams& p, const AttnScratch& scratch, bool bwd, int force = ATTN_ANY);

// ---- tile forms: one row per head dim ---------------------------------------------------------------------------------------------
// forward attn_fwd_kernel<D, QT, KT, DSPLIT> / attn_fwd_dma_kernel<D, QT, KT, NW>: a wave owns QT 16-query tiles, KT keys per tile; DSPLIT 4:
// the four waves share the query tiles and split the head dim (d = 512: 64 queries per workgroup, K/V stream traffic per query / 4).
// dQ attn_bwd_dq_kernel<D, QT, KT, DSPLIT>; dK/dV attn_bwd_dkv_kernel<D, KTW, QTL, DSPLIT>: KTW 16-key tiles per wave, QTL queries per tile.
// sk_nw: waves of attn_fwd_shortk_kernel<D, NW> (0: none for this head dim).  fp8: the row of AttnParams::pv_fp8 (128-key tiles, 8 waves,
// forward only); attn_form_of never returns it.
struct AttnForm {
  int d, qt, kt, dsplit, dq_qt, dq_kt, ktw, qtl, sk_nw;
  bool fp8;
  // LDS-DMA staging: head dims whose rows are whole 16-byte granules and whose tiles are whole 1 KB pieces (d = 160: the two-deep ring
  // would cost a workgroup per CU); 8 waves at d <= 40 when the queries fill them
  constexpr bool dma() const { return dsplit == 1 && d % 8 == 0 && d <= 80; }
  constexpr bool dma8() const { return dma() && d <= 40; }
};
constexpr AttnForm ATTN_FORMS[] = {
    {32, 2, 64, 1, 2, 64, 2, 64, 0, false},
    {40, 2, 64, 1, 2, 64, 2, 64, 8, false},
    {64, 2, 64, 1, 2, 64, 2, 64, 4, false},
    {80, 2, 64, 1, 1, 64, 1, 64, 4, false},
    {160, 2, 64, 1, 1, 64, 1, 64, 0, false},
    {512, 4, 32, 4, 1, 32, 1, 32, 0, false},
    {64, 2, 128, 1, 0, 0, 0, 0, 0, true},
};
constexpr int ATTN_NFORMS = sizeof(ATTN_FORMS) / sizeof(ATTN_FORMS[0]);
constexpr int ATTN_FORM_FP8 = ATTN_NFORMS - 1;
inline int attn_form_of(int d) {
  for (int i = 0; i < ATTN_NFORMS; ++i)
    if (ATTN_FORMS[i].d == d && !ATTN_FORMS[i].fp8) return i;
  return -1;
}
// the one switch from a row to template instantiations: f(std::integral_constant<int, row>) with ATTN_FORMS[row] a constant expression
template <class F>
hipError_t attn_with_form(int form, F&& f) {
  switch (form) {
    case 0: return f(std::integral_constant<int, 0>{});
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    default: return hipErrorInvalidValue;
  }
}
static_assert(ATTN_NFORMS == 7, "attn_with_form lists the rows");

// ---- predicates the planner, the scratch sizing and the units share -----------------------------------------------------------------
// rows of one image within the 32-bit byte offsets of the LDS-DMA (buffer) loads
inline bool offsets_fit_32bit(int rows, int ld) { return (size_t)rows * (size_t)ld * 2 < 0xF0000000ull; }
// the GEMM route's shapes: wide heads, whole 64 x 64 score tiles, no mask
inline bool attn_gemm_shape(int Nq, int Nk, int D, bool causal) { return D >= 256 && (D % 64) == 0 && (Nq % 64) == 0 && (Nk % 64) == 0 && !causal; }
// ... and the most images it takes per launch: single-head layers only (with H > 1 the heads of one image interleave along the columns of
// the same rows, so the images of a group do not stack along M), whole 256-row tiles per image
inline int attn_gemm_group_max(int B, int H, int Nq, int Nk) { return (H != 1 || (Nq & 255) || (Nk & 255)) ? 1 : (B < 8 ? (B < 1 ? 1 : B) : 8); }

// ---- what the units offer the launcher: they act on a plan and check nothing ----------------------------------------------------------
hipError_t launch_attention_shortk(const AttnParams& p, const AttnPlan& plan, hipStream_t stream);                            // attention_shortk.hip
hipError_t launch_attention_gemm(const AttnParams& p, const AttnScratch& scratch, int group, bool bwd, hipStream_t stream);   // attention_gemm.hip

// ---- environment switch of the family, read once per process on first use ------------------------------------------------------------
struct AttnEnv {
  int shortk;          // DD_ATTN_SHORTK (default 1): 0 keeps <= 80-key launches on the streaming forward
};
inline const AttnEnv& attn_env() {
  static const AttnEnv e = [] { const char* v = getenv("DD_ATTN_SHORTK"); return AttnEnv{v ? atoi(v) : 1}; }();
  return e;
}
