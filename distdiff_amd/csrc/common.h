// Common device/host helpers for the distdiff_amd HIP kernels (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The 16-bit storage format of activations, weights and gradients is fixed when the library is compiled: bf16 (the product library),
// or IEEE half with -DDD_ACT_F16 (libdistdiff_hip_f16.so).  It lives in this block alone: the raw storage type, the five conversions,
// the MFMA operand vector with its instruction, and the constant 1.0.  bf16_t names the raw 16 bits in either build.
typedef unsigned short bf16_t;  // raw 16-bit storage (bf16, or fp16 under DD_ACT_F16)
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef float f32x2_t __attribute__((ext_vector_type(2)));

#define DD_WAVE 64

#ifdef DD_ACT_F16
#define DD_ACT_DTYPE 1
#define DD_ACT_ONE 0x3c00u      // 1.0
typedef __attribute__((ext_vector_type(8))) _Float16 bf16x8;
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
// v_cvt_f32_f16 / v_cvt_pk_f16_f32: RNE, NaN preserved, no saturation (beyond 65504 -> inf); never cvt_pkrtz, which rounds toward zero
__device__ __forceinline__ float bf2f(bf16_t v) { return (float)__builtin_bit_cast(_Float16, v); }
__device__ __forceinline__ bf16_t f2bf(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f); }
__device__ __forceinline__ unsigned pack2bf(float lo, float hi) {
  const f32x2_t v = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2_t));
}
// one dword of two stored values -> two floats (lo in bits 0-15)
__device__ __forceinline__ void unpack2(unsigned u, float& lo, float& hi) {
  const f32x2_t v = __builtin_convertvector(__builtin_bit_cast(f16x2_t, u), f32x2_t);
  lo = v[0]; hi = v[1];
}
__device__ __forceinline__ void unpack8(const uint4& v, float* f) {
  unpack2(v.x, f[0], f[1]); unpack2(v.y, f[2], f[3]); unpack2(v.z, f[4], f[5]); unpack2(v.w, f[6], f[7]);
}
// the one MFMA of the 16-bit kernels (a macro: the bf16 build must compile to the code it was before the two formats shared it)
#define mfma16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0)
#else
#define DD_ACT_DTYPE 0
#define DD_ACT_ONE 0x3f80u      // 1.0
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
__device__ __forceinline__ float bf2f(bf16_t v) { return __uint_as_float(((unsigned)v) << 16); }
__device__ __forceinline__ bf16_t f2bf(float f) {
  __bf16 h = (__bf16)f;  // v_cvt_pk_bf16_f32: RNE, NaN preserved
  return __builtin_bit_cast(unsigned short, h);
}
// two floats -> one dword of two bf16 (lo in bits 0-15): a single v_cvt_pk_bf16_f32 (RNE), not two conversions + shift + or
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pack2bf(float lo, float hi) {
  const f32x2_t v = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
}
// one dword of two stored values -> two floats (lo in bits 0-15)
__device__ __forceinline__ void unpack2(unsigned u, float& lo, float& hi) {
  lo = __uint_as_float(u << 16); hi = __uint_as_float(u & 0xffff0000u);
}
__device__ __forceinline__ void unpack8(const uint4& v, float* f) {
  f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
  f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
  f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xffff0000u);
  f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xffff0000u);
}
#define mfma16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0)
#endif
__device__ __forceinline__ uint4 pack8(const float* f) {
  uint4 v; v.x = pack2bf(f[0], f[1]); v.y = pack2bf(f[2], f[3]); v.z = pack2bf(f[4], f[5]); v.w = pack2bf(f[6], f[7]);
  return v;
}
// the residual of four output columns, two dwords of stored values, added to their fp32 sums (the conv / GEMM epilogues; a macro for the
// reason given at DD_STORED4 below)
#ifdef DD_ACT_F16
#define add_res4(q0, q1, v0, v1, v2, v3)                        \
  do {                                                          \
    float lo_, hi_;                                             \
    unpack2(q0, lo_, hi_); v0 += lo_; v1 += hi_;                \
    unpack2(q1, lo_, hi_); v2 += lo_; v3 += hi_;                \
  } while (0)
#else
#define add_res4(q0, q1, v0, v1, v2, v3)                                                 \
  do {                                                                                   \
    v0 += __uint_as_float((q0) << 16); v1 += __uint_as_float((q0) & 0xffff0000u);        \
    v2 += __uint_as_float((q1) << 16); v3 += __uint_as_float((q1) & 0xffff0000u);        \
  } while (0)
#endif
// What the CF_STATS partials sum for four values on their way to a 16-bit store.  The fp16 build sums the values the tensor STORES (the
// rounded ones, read back from the very dwords the epilogue writes: the compiler shares the two packs with the store), so the GroupNorm
// that merges the partials normalises the tensor with that tensor's own statistics.  The bf16 build sums the fp32 values in front of the
// rounding, as it always has: its bits are the record the bit tests compare with.
// (a macro that declares u0 .. u3: as a function with reference results it moved the bf16 build's epilogue schedule)
#ifdef DD_ACT_F16
#define DD_STORED4(v0, v1, v2, v3, u0, u1, u2, u3) \
  float u0, u1, u2, u3;                            \
  unpack2(pack2bf(v0, v1), u0, u1);                \
  unpack2(pack2bf(v2, v3), u2, u3)
#else
#define DD_STORED4(v0, v1, v2, v3, u0, u1, u2, u3) const float u0 = (v0), u1 = (v1), u2 = (v2), u3 = (v3)
#endif
// Cotangent normalisation of the fp16 build.  A reverse program is linear in its cotangent, is entered from an fp32
// tensor and left into one: the entry kernel multiplies by a power of two s that puts the cotangent's absolute maximum into
// [2^7, 2^8) -- 2^8 below the largest half for growth inside the program, 21 binades of normal range below the maximum -- and the exit
// kernel by 1 / s, both exact.  s lives in a device scalar (launch_cot_scale, elementwise.hip); CotScale is how those kernels see it.
// The bf16 build has bf16's fp32 exponent range and none of this: its CotScale is empty and mul() is the constant 1.
#ifdef DD_ACT_F16
struct CotScale {
  const float* p;
  __device__ __forceinline__ float mul() const { return p ? *p : 1.f; }
};
inline CotScale cot_scale_arg(const float* p) { return CotScale{p}; }
#else
struct CotScale {
  __device__ __forceinline__ float mul() const { return 1.f; }
};
inline CotScale cot_scale_arg(const float*) { return CotScale{}; }
#endif
// A row of T (bf16_t or float) as the side kernels see it: one 16-byte vector holds V = 1 << SH elements, which are fp32 between
// ld and st; get / put move one element.  bf16 rounds in st / put (RNE), fp32 is stored as it is.
template <typename T> struct Row;
template <> struct Row<bf16_t> {
  static constexpr int SH = 3, V = 8;
  static __device__ __forceinline__ void ld(const bf16_t* p, float* f) { unpack8(*(const uint4*)p, f); }
  static __device__ __forceinline__ void st(bf16_t* p, const float* f) { *(uint4*)p = pack8(f); }
  static __device__ __forceinline__ float get(const bf16_t* p) { return bf2f(*p); }
  static __device__ __forceinline__ void put(bf16_t* p, float v) { *p = f2bf(v); }
};
template <> struct Row<float> {
  static constexpr int SH = 2, V = 4;
  static __device__ __forceinline__ void ld(const float* p, float* f) {
    const float4 v = *(const float4*)p;
    f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
  }
  static __device__ __forceinline__ void st(float* p, const float* f) { *(float4*)p = make_float4(f[0], f[1], f[2], f[3]); }
  static __device__ __forceinline__ float get(const float* p) { return *p; }
  static __device__ __forceinline__ void put(float* p, float v) { *p = v; }
};
// v_rcp_f32 (1 ulp) instead of the IEEE division sequence (~10 VALU per element: GroupNorm+SiLU touches every activation)
__device__ __forceinline__ float silu_f(float x) { return x * __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
__device__ __forceinline__ float dsilu_f(float x) { float s = __builtin_amdgcn_rcpf(1.f + __expf(-x)); return s * (1.f + x * (1.f - s)); }
// erf-GELU (torch default, approximate='none') and its derivative
// erf for the GEGLU epilogue: Abramowitz-Stegun 7.1.26, branch-free (rcp + exp2 + 6 fma), |error| <= 5e-7 in fp32 -- four orders of
// magnitude below the bf16 rounding of the result (the reference evaluates GELU in fp16).  The library erff costs ~3x the VALU and the
// 5-step GEGLU items are epilogue-bound (conv family -14 ms per bench step, tools/ab_ops.sh).  The exact erff stays in dgelu_f.
__device__ __forceinline__ float erf_as(float x) {
  const float ax = fabsf(x);
  const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(0.3275911f, ax, 1.f));
  float p = __builtin_fmaf(1.061405429f, t, -1.453152027f);
  p = __builtin_fmaf(p, t, 1.421413741f);
  p = __builtin_fmaf(p, t, -0.284496736f);
  p = __builtin_fmaf(p, t, 0.254829592f);
  const float e = __builtin_amdgcn_exp2f(ax * ax * -1.4426950408889634f);
  return copysignf(__builtin_fmaf(-p * t, e, 1.f), x);
}
__device__ __forceinline__ float gelu_erf_f(float x) { return 0.5f * x * (1.f + erf_as(x * 0.70710678118654752f)); }
// GELU for the GEGLU epilogues WITHOUT transcendentals: gelu(x) = x * Phi(x), Phi(x) ~ 0.5 + t * P(t^2) with t = clamp(x, -4.5, 4.5) and P
// the degree-9 minimax polynomial (10 coefficients, fitted by linear programming under the constraint Phi~(4.5) = 1, so that the
// clamped ends are exactly 0 / 1).  13 full-rate VALU (v_med3, v_mul, 9 v_fma, v_fma, v_mul) instead of ~20 + v_rcp + v_exp: the K = 320
// GEGLU projection is bound by the vector issue port (an MFMA holds it for 8 of its 16 cycles, MI355X guide), not by the matrix pipe.
// Accuracy (tests/test_oracle.py::test_gelu_polynomial, evaluated in fp32 from THESE literals): |gelu~ - gelu| <= 5e-5 everywhere,
// relative error <= 1.2e-5 for x > 0 and <= 1e-4 for x > -2; beyond -3 the value itself is < 4e-3 and only the absolute bound holds.
// One bf16 rounding of the product is 2e-3 relative: 0.1 / 0.4 / 6.8 % of the bf16 outputs differ from the rounded exact product for
// gate pre-activations of sigma 0.5 / 1 / 2 (A&S form above: 0.003 / 0.009 / 1.4 %), by one ulp except in the tail.
#define DD_GELU_CLAMP 4.5f
#define DD_GELU_POLY { 3.989228904e-01f, -6.641460210e-02f, 9.885823354e-03f, -1.140101929e-03f, 1.011194836e-04f, \
                       -6.729636425e-06f, 3.209943316e-07f, -1.023312812e-08f, 1.934523375e-10f, -1.629367648e-12f }
__device__ __forceinline__ float gelu_poly_f(float x) {
  constexpr float c[10] = DD_GELU_POLY;
  const float t = __builtin_amdgcn_fmed3f(x, -DD_GELU_CLAMP, DD_GELU_CLAMP);
  const float u = t * t;
  float p = c[9];
#pragma unroll
  for (int k = 8; k >= 0; --k) p = __builtin_fmaf(p, u, c[k]);
  return x * __builtin_fmaf(t, p, 0.5f);
}
#ifdef DD_GELU_ERF_AS      // A/B build: the rcp + exp2 form in the epilogues
__device__ __forceinline__ float gelu_f(float x) { return gelu_erf_f(x); }
#else
__device__ __forceinline__ float gelu_f(float x) { return gelu_poly_f(x); }
#endif
__device__ __forceinline__ float dgelu_f(float x) {
  return 0.5f * (1.f + erff(x * 0.70710678118654752f)) + x * 0.3989422804014327f * __expf(-0.5f * x * x);
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// One 1 KB LDS-DMA piece: buffer_load_dwordx4 ... lds from base + voff (per lane) + soff (scalar); a lane whose voff is beyond the
// 4 GB - 256 B range gets zeros written to its LDS slot (hardware range check) -- that is how padding taps and ragged rows are
// staged.  The resource builtins only exist in the device pass (a kernel template that names them loses its host stub otherwise).
__device__ __forceinline__ void dma16(const void* base, void* lds, unsigned voff, unsigned soff) {
#if defined(__HIP_DEVICE_COMPILE__)
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 0xffffff00u, 0x00020000);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds, 16, voff, soff, 0, 0);
#endif
}

// sum over the 16 lanes of a DPP row (the 16 pixel rows of an MFMA tile); every lane of the row receives the total
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float row16_sum(float v) {
  v = dpp_add<0xB1>(v);    // quad_perm [1,0,3,2]
  v = dpp_add<0x4E>(v);    // quad_perm [2,3,0,1]
  v = dpp_add<0x141>(v);   // row_half_mirror
  v = dpp_add<0x140>(v);   // row_mirror
  return v;
}

// Host: grid of the persistent kernels that run one workgroup per CU -- the device's CU count rounded down to whole XCD rounds of 8
// (256 on an MI355X, which is also what a process without a device plans with).  Read once per process.
inline int persistent_cus() {
  static const int cus = [] { int d = 0, n = 256; (void)hipGetDevice(&d); (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d); return n > 8 ? n & ~7 : 8; }();
  return cus;
}
// Device: the tiles of the XCD that workgroup `block` runs on.  Workgroups b, b + 8, ... share an XCD, and every XCD owns one contiguous
// range of the `tiles` (n-tiles fastest inside it, so that its L2 holds the operands they share): first tile and length of that range.
struct XcdRange { int first, count; };
__device__ __forceinline__ XcdRange xcd_tile_range(int tiles, int block) {
  const int q = tiles >> 3, r = tiles & 7, xcd = block & 7;
  return {xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q, q + (xcd < r ? 1 : 0)};
}
