// Private to the flash attention kernels (attention.hip: attn_fwd_kernel, attn_fwd_dma_kernel, attn_bwd_dq_kernel, attn_bwd_dkv_kernel;
// attention_shortk.hip: attn_fwd_shortk_kernel): the steps those kernels share, written once -- the tile geometry, the LDS fragment reads,
// the register-staged tile loads and stores, the owner rows, the score chains, the key mask, the softmax pieces, the P.V loop, the row
// sum, the row epilogue and the fp8 P.V -- and the launch helper for kernels with dynamic LDS.  Who uses what, and what was measured
// where a kernel keeps a text of its own (profiles/attention_kernels_unified.json has the numbers):
//   attn_fwd_kernel, attn_fwd_dma_kernel   every piece
//   attn_bwd_dq_kernel, attn_bwd_dkv_kernel   geometry, fragments, staging functions, owner rows, row epilogue.  Their two score chains and
//       two column loops run MFMA by MFMA in turn and stay in the kernels: as calls of score_chains / colfrag_mfma they lost up to 14 %.
//   the staging loop (load ahead, barrier, store or stage, barrier) is spelled in each of the three register-staged kernels: as one
//       object with prime / publish / fetch_next it cost the d = 512 backward kernels 0.3 - 0.9 % (direct staging), beyond their margin
//   attn_fwd_shortk_kernel   geometry and fragments only: on the shared scores / mask / softmax / P.V / epilogue it needed 40 fewer
//       registers at d = 80 but d = 64 ran 1.2 % slower, and with P.V per query tile all three head dims did
// The layout these helpers assume is described at the top of attention.hip.  Every device helper is force-inlined and fully unrolled: an
// instantiation sees straight-line code.
#pragma once
#include <cmath>
#include "common.h"
#include "kernels.h"

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(8))) int i32x8_t;

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

// ---- geometry ------------------------------------------------------------------------------------------------------------------------
// LDS rows of the LDS-DMA staged tiles (attn_fwd_dma_kernel's K / V ring, attn_fwd_shortk_kernel's K, V and Q blocks): RG 16-byte granules,
// DG = D / 8 of them data.  Row strides (96 B at d <= 40, 160 B at d = 64 / 80: no padding granule, or none past column 79: the over-read of
// the last K-step lands in the next row) are bank-conflict free for the ds_read_b128 row fragments and the ds_read_b64_tr_b16 column
// fragments (tools/lds_conflicts.py).  attn_dpk / attn_dma_row_bytes / attn_stream_row_bytes / attn_stream_span: the same numbers for the
// planner's grids and LDS sizes.
constexpr int attn_dpk(int d) { return (d + 31) / 32 * 32; }
constexpr int attn_stream_row_bytes(int d) { return attn_dpk(d) * 2 + 32; }                    // the register-staged kernels' LDS rows
constexpr int attn_stream_span(int dsplit) { return (dsplit == 1 ? 4 : 1) * 16; }              // owner rows of one 16-row tile per wave, over the workgroup
constexpr int attn_dma_row_bytes(int d) { return d <= 40 ? 96 : d <= 80 ? 160 : attn_stream_row_bytes(d); }
// head dims with a padded column inside the last 16-wide output tile (d = 40): that column of V is set to 1.0, so the P.V MFMAs
// also deliver the softmax row sums (of exactly the bf16 P the outputs are built from) and the 16 VALU adds per query tile and
// KV tile disappear -- the forward is VALU-bound at d = 40
constexpr bool attn_ones(int d) { return (d % 16) != 0 && (d % 8) == 0; }
template <int D>
struct AttnLdsGeo {
  static constexpr int DPK = attn_dpk(D);
  static constexpr int RB = attn_dma_row_bytes(D);           // LDS row bytes
  static constexpr int RG = RB / 16, DG = D / 8;             // granules per row, data granules
  static constexpr int KS = DPK / 32, DVT = (D + 15) / 16;
};
// The register-staged kernels (attn_fwd_kernel, attn_bwd_dq_kernel, attn_bwd_dkv_kernel), 256 threads.  DSPLIT = 1: each wave owns T
// 16-row tiles; DSPLIT = 4: the 4 waves share one set of T tiles and each accumulates a quarter of the head dim (d = 512).
template <int D, int DSPLIT>
struct AttnStreamGeo {
  static constexpr int DPK = attn_dpk(D), KS = DPK / 32, DVT = (D + 15) / 16;
  static constexpr int DTW = DVT / DSPLIT;                   // dv tiles per wave
  static constexpr int S = attn_stream_row_bytes(D);
  static __device__ __forceinline__ int row0(int T, int wave) { return blockIdx.x * attn_stream_span(DSPLIT) * T + (DSPLIT == 1 ? wave * T * 16 : 0); }
  static __device__ __forceinline__ int dt0(int wave) { return DSPLIT == 1 ? 0 : wave * DTW; }
};

// ---- fragments -----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bf16x8 lds_row_frag(const unsigned char* base, int row, int S, int slot) {
  return *(const bf16x8*)(base + row * S + slot * 16);
}
// 8 k-values (permuted order, see attention.hip's header) of column `col16 * 16 + (lane&15)`: rows r0 + 4*(lane>>4) + {0..3} and +16
__device__ __forceinline__ bf16x8 lds_col_frag(const unsigned char* base, int r0, int S, int col16, int lane) {
  const int i = lane & 15, g = lane >> 4;
  const unsigned char* a = base + (r0 + 4 * g + (i >> 2)) * S + (col16 * 16 + 4 * (i & 3)) * 2;
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a));
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a + 16 * S));
  s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}
// Maxima of MFMA results as single instructions the COMPILER sees: fmaxf() makes it put a canonicalising v_max_f32 v, v, v in front of
// every operand that comes out of an MFMA, and an inline-asm v_max3_f32 (round 3) is invisible to its hazard recogniser -- nothing then
// guarantees the wait states between an MFMA and a vector instruction that reads its result, and with one MFMA per score tile (d = 32)
// the asm read registers the MFMA had not written yet (NaN outputs; found with tools/attn_dbg.py).  v_med3_f32(a, b, +inf) = max(a, b) is
// a target intrinsic: no canonicalisation, hazards handled.
__device__ __forceinline__ float vmax2(float a, float b) { return __builtin_amdgcn_fmed3f(a, b, __builtin_inff()); }
__device__ __forceinline__ float vmax3(float a, float b, float c) { return vmax2(vmax2(a, b), c); }
__device__ __forceinline__ bf16x8 pack_frag(const f32x4& a, const f32x4& b) {
  uint4 u;
  u.x = pack2bf(a[0], a[1]); u.y = pack2bf(a[2], a[3]); u.z = pack2bf(b[0], b[1]); u.w = pack2bf(b[2], b[3]);
  return __builtin_bit_cast(bf16x8, u);
}

// ---- owner rows: the rows a lane owns on the MFMA column (Q of the forward kernels, Q and dO of dQ, K and V of dK/dV) ----------------
struct OwnerRow {
  int row, nrows;
  __device__ __forceinline__ bool valid() const { return row < nrows; }
};
__device__ __forceinline__ OwnerRow owner_row(int row0, int nrows, int lane) { return OwnerRow{row0 + (lane & 15), nrows}; }
template <int DPK>
__device__ __forceinline__ void load_row_frags(bf16x8* f, const bf16_t* g, bool valid, int D, int lane) {
  const int gq = lane >> 4;
#pragma unroll
  for (int ks = 0; ks < DPK / 32; ++ks) {
    const int d0 = ks * 32 + gq * 8;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (valid && d0 < D) v = *(const uint4*)(g + d0);
    f[ks] = __builtin_bit_cast(bf16x8, v);
  }
}
// fragments of owner row r of head h of image b in a [B * nrows, ld] matrix (zeros for an invalid row)
template <int D>
__device__ __forceinline__ void owner_frags(bf16x8* f, const bf16_t* m, int ld, int nrows, int b, int h, const OwnerRow& r, int lane) {
  load_row_frags<attn_dpk(D)>(f, m + ((size_t)b * nrows + (r.valid() ? r.row : 0)) * ld + h * D, r.valid(), D, lane);
}

// ---- register-staged tiles (attn_fwd_kernel, attn_bwd_dq_kernel, attn_bwd_dkv_kernel) ------------------------------------------------------
// stage ROWS x DPK bf16 (zero padded beyond D columns / nvalid rows) into LDS with row stride S bytes
// ONES: column D of the tile (a padding column) is set to 1.0, so that P.V also accumulates the softmax row sums (forward V tile)
template <int ROWS, int DPK, bool ONES = false>
__device__ __forceinline__ void stage_tile(unsigned char* lds, int S, const bf16_t* g, int ld, int nvalid, int D, int tid) {
  constexpr int VPR = DPK / 8;
  for (int idx = tid; idx < ROWS * VPR; idx += 256) {
    const int r = idx / VPR, v = idx % VPR;
    uint4 val = make_uint4(0, 0, 0, 0);
    if (r < nvalid && v * 8 < D) val = *(const uint4*)(g + (size_t)r * ld + v * 8);
    if (ONES && v * 8 == D) val.x = DD_ACT_ONE;
    *(uint4*)(lds + r * S + v * 16) = val;
  }
}
// register-staged variant: issue the global loads of a tile early, write them to LDS after the compute of the previous tile
template <int ROWS, int DPK>
struct TileRegs { uint4 v[(ROWS * (DPK / 8) + 255) / 256]; };
template <int ROWS, int DPK, bool ONES = false>
__device__ __forceinline__ void tile_load(TileRegs<ROWS, DPK>& t, const bf16_t* g, int ld, int nvalid, int D, int tid) {
  constexpr int VPR = DPK / 8, N = (ROWS * VPR + 255) / 256;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int idx = tid + i * 256;
    const int r = idx / VPR, v = idx % VPR;
    uint4 val = make_uint4(0, 0, 0, 0);
    if (idx < ROWS * VPR && r < nvalid && v * 8 < D) val = *(const uint4*)(g + (size_t)r * ld + v * 8);
    if (ONES && v * 8 == D) val.x = DD_ACT_ONE;
    t.v[i] = val;
  }
}
template <int ROWS, int DPK>
__device__ __forceinline__ void tile_store(const TileRegs<ROWS, DPK>& t, unsigned char* lds, int S, int tid) {
  constexpr int VPR = DPK / 8, N = (ROWS * VPR + 255) / 256;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int idx = tid + i * 256;
    const int r = idx / VPR, v = idx % VPR;
    if (idx < ROWS * VPR) *(uint4*)(lds + r * S + v * 16) = t.v[i];
  }
}

// ---- scores --------------------------------------------------------------------------------------------------------------------------
// S^T = L O^T: NL 16-row tiles of the LDS tile Ls against the fragments of NO owner tiles; every chain starts from init(owner tile, LDS
// tile) -- zero, or minus the lazy reference.  Lane (i16, g) then holds, for owner row i16 of tile o, LDS rows 16 l + 4 g + {0 .. 3}.
template <int NO, int NL, int KS, class Init>
__device__ __forceinline__ void score_chains(f32x4 (&st)[NO][NL], const unsigned char* Ls, int S, const bf16x8 (&of)[NO][KS], int lane, Init&& init) {
  const int i16 = lane & 15, g = lane >> 4;
#pragma unroll
  for (int l = 0; l < NL; ++l) {
#pragma unroll
    for (int o = 0; o < NO; ++o) st[o][l] = init(o, l);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const bf16x8 lf = lds_row_frag(Ls, l * 16 + i16, S, g + 4 * ks);
#pragma unroll
      for (int o = 0; o < NO; ++o) st[o][l] = mfma16(lf, of[o][ks], st[o][l]);
    }
  }
}
__device__ __forceinline__ f32x4 splat4(float x) { return f32x4{x, x, x, x}; }

// ---- softmax pieces (one owner tile: st[kt][r] = score of key k0 + 16 kt + 4 g + r) --------------------------------------------------
// keys from klim on leave the softmax
template <int NKT>
__device__ __forceinline__ void mask_keys(f32x4 (&st)[NKT], int k0, int klim, int g) {
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (k0 + kt * 16 + 4 * g + r >= klim) st[kt][r] = -INFINITY;
}
template <int NKT>
__device__ __forceinline__ float row_max(const f32x4 (&st)[NKT]) {
  float mx = vmax3(st[0][0], st[0][1], st[0][2]);
  mx = vmax2(mx, st[0][3]);
#pragma unroll
  for (int kt = 1; kt < NKT; ++kt) {
    mx = vmax3(mx, st[kt][0], st[kt][1]);
    mx = vmax3(mx, st[kt][2], st[kt][3]);
  }
  mx = vmax2(mx, __shfl_xor(mx, 16, 64));
  return vmax2(mx, __shfl_xor(mx, 32, 64));
}
// st <- exp2(st * c - m) (FMA = false: exp2(st), the scores already are log2-domain differences); returns this lane's part of the row sum
// (kt outer, r inner: the order fixes its bits), 0 with ONES (the sum then comes out of P.V)
template <bool FMA, bool ONES, int NKT>
__device__ __forceinline__ float exp2_scores(f32x4 (&st)[NKT], float c, float m) {
  float ps = 0.f;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float e = __builtin_amdgcn_exp2f(FMA ? __builtin_fmaf(st[kt][r], c, -m) : st[kt][r]);
      st[kt][r] = e;
      if (!ONES) ps += e;
    }
  return ps;
}
// one online-softmax step of one owner tile: scores -> probabilities, running maximum, row sum and O rescaled
// softmax is VALU-bound at d = 40 (one exp per score): keep it to max + fma + exp + add per element
template <bool ONES, int NKT, int DT>
__device__ __forceinline__ void online_softmax(f32x4 (&st)[NKT], float& mrun, float& lsum, f32x4 (&o)[DT], float sl2) {
  const float mnew = vmax2(mrun, row_max(st) * sl2);         // running max in the scaled log2 domain (sl2 > 0)
  const float alpha = __builtin_amdgcn_exp2f(mrun - mnew);
  const float ps = exp2_scores<true, ONES>(st, sl2, mnew);
  if (!ONES) lsum = lsum * alpha + ps;
  mrun = mnew;
  if (__any(alpha != 1.f)) {                                 // wave-uniform: skip the O rescale when no row max moved
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] *= alpha;
  }
}
template <int NKT>
__device__ __forceinline__ void pack_probs(bf16x8 (&pf)[NKT / 2], const f32x4 (&st)[NKT]) {
#pragma unroll
  for (int c = 0; c < NKT / 2; ++c) pf[c] = pack_frag(st[2 * c], st[2 * c + 1]);
}

// ---- P.V: acc[o][dt] += column fragments (dv tile dt0 + dt) of the LDS tile x the packed score fragments --------
template <int NO, int NC, int DT>
__device__ __forceinline__ void colfrag_mfma(f32x4 (&acc)[NO][DT], const unsigned char* Vs, int S, const bf16x8 (&pf)[NO][NC], int dt0, int lane) {
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const bf16x8 vf = lds_col_frag(Vs, 32 * c, S, dt0 + dt, lane);
#pragma unroll
      for (int o = 0; o < NO; ++o) acc[o][dt] = mfma16(vf, pf[o][c], acc[o][dt]);
    }
}

// ---- row sum, row epilogue -------------------------------------------------------------------------------------------------------------
// ONES (d % 16 == 8, d = 40): column D of the staged V is 1.0, so P.V delivered the sum of the bf16-ROUNDED probabilities in O column D --
// output row D % 16 of the last tile = lane group (D % 16) / 4, register (D % 16) % 4: O is then an exact convex combination of the value
// rows; else the fp32 sum of the unrounded probabilities, this lane's part `part` completed by two shuffles
template <int D, bool ONES>
__device__ __forceinline__ float row_sum(float part, const f32x4& olast, int lane) {
  if (ONES) return __shfl(olast[(D % 16) % 4], ((D % 16) / 4) * 16 + (lane & 15), 64);
  part += __shfl_xor(part, 16, 64);
  return part + __shfl_xor(part, 32, 64);
}
// One owner row of an output matrix: acc * mul (1 / l, the scale, or 1 for dV) as bf16 to columns (dt0 + dt) * 16 + 4 g + {0 .. 3} (g: the
// lane group, lane >> 4) of `row` (the row's head: row + h * D).  hipcc lowers every `if (dv < D)` here to ONE lane-predicated
// global_store_dwordx2 (D % 16 != 0: the lanes behind D store nothing).  That is an expectation about the generated code, not a property of
// this source; a kernel with hand-counted vmcnt waits (attn_fwd_shortk_kernel counts 2 DVT O stores per 32-query tile in its own epilogue
// of the same shape) must check the ISA before it relies on it.
template <int D, int DT>
__device__ __forceinline__ void store_row(bf16_t* row, const f32x4 (&acc)[DT], float mul, int dt0, int g) {
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    const int dv = (dt0 + dt) * 16 + 4 * g;
    if (dv < D) *(uint2*)(row + dv) = make_uint2(pack2bf(acc[dt][0] * mul, acc[dt][1] * mul), pack2bf(acc[dt][2] * mul, acc[dt][3] * mul));
  }
}
// LSE fp32 [B][H][Nq], natural-log domain, from the log2-domain maximum (or reference) m2 and the row sum l; one lane group writes
__device__ __forceinline__ void store_lse(const AttnParams& p, int b, int h, int qrow, float m2, float l, bool writer) {
  if (p.lse && writer) p.lse[((size_t)b * p.H + h) * p.Nq + qrow] = (m2 + log2f(l)) * LN2;
}

// ---- fp8 P.V (attn_fwd_dma_kernel<.., FP8>: d = 64, 128-key tiles) ---------------------------------------------------------------------
// V tile -> e4m3 in the operand order of the probabilities: dword ((dt * 4 + g) * 16 + i16) * 8 + kt = V[16 kt + 4 g + r][16 dt + i16], r = 0 .. 3
template <int NT>
__device__ __forceinline__ void fp8_quantise_v(unsigned char* VQ, const unsigned char* Vs, int S, int tid) {
  for (int w = tid; w < 64 * 4 * 8; w += NT) {
    const int kt = w & 7, d = ((w >> 9) << 4) + ((w >> 3) & 15), gg = (w >> 7) & 3;
    const unsigned char* src = Vs + (16 * kt + 4 * gg) * S + d * 2;
    const float f0 = bf2f(*(const bf16_t*)src), f1 = bf2f(*(const bf16_t*)(src + S)), f2 = bf2f(*(const bf16_t*)(src + 2 * S)), f3 = bf2f(*(const bf16_t*)(src + 3 * S));
    int wv = __builtin_amdgcn_cvt_pk_fp8_f32(f0, f1, 0, false);
    wv = __builtin_amdgcn_cvt_pk_fp8_f32(f2, f3, wv, true);
    *(int*)(VQ + w * 4) = wv;
  }
}
// the probabilities of one owner tile, four keys per dword straight from the score accumulators: the instruction's 32-byte operand
template <int NKT>
__device__ __forceinline__ i32x8_t fp8_pack_probs(const f32x4 (&st)[NKT]) {
  static_assert(NKT == 8, "128-key tiles");
  i32x8_t pf8;
#pragma unroll
  for (int kt = 0; kt < 8; ++kt) {
    const int lo = __builtin_amdgcn_cvt_pk_fp8_f32(st[kt][0], st[kt][1], 0, false);
    pf8[kt] = __builtin_amdgcn_cvt_pk_fp8_f32(st[kt][2], st[kt][3], lo, true);
  }
  return pf8;
}
// o[qt][dt] += e4m3 V (fp8_quantise_v's tile, published by a barrier) x e4m3 probabilities, unit block scales, 128 keys per instruction
template <int QT, int DVT>
__device__ __forceinline__ void fp8_pv(f32x4 (&o)[QT][DVT], const unsigned char* VQ, const i32x8_t (&pf8)[QT], int lane) {
#pragma unroll
  for (int dt = 0; dt < DVT; ++dt) {
    const unsigned char* vq = VQ + ((dt * 4 + (lane >> 4)) * 16 + (lane & 15)) * 32;
    const uint4 v0 = *(const uint4*)vq, v1 = *(const uint4*)(vq + 16);
    const i32x8_t vf8 = {(int)v0.x, (int)v0.y, (int)v0.z, (int)v0.w, (int)v1.x, (int)v1.y, (int)v1.z, (int)v1.w};
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
      o[qt][dt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(vf8, pf8[qt], o[qt][dt], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
  }
}

// Launch of a kernel with dynamic LDS: the first launch of every kernel raises its limit (lds is a constant of the instantiation)
template <auto KERNEL, class... Args>
hipError_t launch_dyn_lds(dim3 grid, dim3 block, size_t lds, hipStream_t s, Args... args) {
  static bool attr = false;
  if (!attr) { (void)hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); attr = true; }
  hipLaunchKernelGGL(KERNEL, grid, block, lds, s, args...);
  return hipGetLastError();
}
