// Private to the attention kernels (attention.hip, attention_shortk.hip): the LDS fragment reads, the LDS row geometry of the LDS-DMA staged
// tiles, and the launch helper for kernels with dynamic LDS.  The layout these helpers assume is described at the top of attention.hip.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;

constexpr float LOG2E = 1.4426950408889634f;

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

// LDS rows of the LDS-DMA staged tiles (attn_fwd_dma_kernel's K / V ring, attn_fwd_shortk_kernel's K, V and Q blocks): RG 16-byte granules,
// DG = D / 8 of them data.  Row strides (96 B at d <= 40, 160 B at d = 64 / 80: no padding granule, or none past column 79: the over-read of
// the last K-step lands in the next row) are bank-conflict free for the ds_read_b128 row fragments and the ds_read_b64_tr_b16 column
// fragments (tools/lds_conflicts.py).  attn_dpk / attn_dma_row_bytes: the same numbers for the planner's LDS sizes.
constexpr int attn_dpk(int d) { return (d + 31) / 32 * 32; }
constexpr int attn_dma_row_bytes(int d) { return d <= 40 ? 96 : d <= 80 ? 160 : attn_dpk(d) * 2 + 32; }
template <int D>
struct AttnLdsGeo {
  static constexpr int DPK = attn_dpk(D);
  static constexpr int RB = attn_dma_row_bytes(D);           // LDS row bytes
  static constexpr int RG = RB / 16, DG = D / 8;             // granules per row, data granules
  static constexpr int KS = DPK / 32, DVT = (D + 15) / 16;
};

// Launch of a kernel with dynamic LDS: the first launch of every kernel raises its limit (lds is a constant of the instantiation)
template <auto KERNEL, class... Args>
hipError_t launch_dyn_lds(dim3 grid, dim3 block, size_t lds, hipStream_t s, Args... args) {
  static bool attr = false;
  if (!attr) { (void)hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); attr = true; }
  hipLaunchKernelGGL(KERNEL, grid, block, lds, s, args...);
  return hipGetLastError();
}
