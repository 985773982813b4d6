// The guide network in exact fp32 (gfx950): implicit-GEMM convolution on v_mfma_f32_32x32x2_f32.  The guide's side kernels (max-pool,
// GAP, bicubic 224 resize and their transposes, ReLU masks, fan-in adds) are the float instances of the row kernels in elementwise.hip.
//
// Why fp32: image_encoder.encode_image (model_utils.py:29-41) is a ReLU / max-pool network, and the energy gradient
// torch.autograd.grad(E, [e, b]) / (E, z) (generate_data.py:721, :761) goes through its ReLU masks.  The gradient of such a
// network is piecewise constant in the input: a forward rounding of 2^-9 (bf16) flips the masks of every activation within that
// distance of zero and moves the input-gradient by 20-30 % (measured against the fp32 oracle, tests/test_guide_f32_gpu.py), while
// the whole guide is < 0.1 % of the FLOPs of an expansion.  So the guide forward, its masks and its VJP run in fp32:
// v_mfma_f32_32x32x2_f32 is an exact k-ordered fmaf chain (1/16 of the bf16 MFMA rate, 157 TFLOP/s peak).
//
// Layout: activations NHWC fp32 rows [pixels, ld] (ld % 4 == 0), weights packed [N][K] fp32 with k = (tap, cin), cin padded to
// a multiple of 4, K padded to 16; the same tap table / stride / dilated-gather conventions as conv_gemm.hip, so the dgrad of a
// stride-2 convolution is the same kernel on the transposed + flipped packing.  Grouped convolutions (ResNeXt, model_utils.py:56-63)
// use the dense block-diagonal packing and skip the K-steps whose channels lie outside the groups of the workgroup's output columns.
// Tile 64 x 64 x 16 per 256-thread workgroup, one 32x32 accumulator per wave, LDS K-major ([k][row], row stride 68 floats:
// staging writes and fragment reads are both bank-conflict free), register-staged prefetch of the next K-step under the MFMAs.
// The MFMA is issued swapped (A = weights, B = pixels) so a lane owns 4 consecutive output channels of one pixel (float4 epilogue).
#include <cstdlib>
#include "common.h"
#include "kernels.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

__global__ __launch_bounds__(256) void conv_f32_kernel(ConvF32Params p) {
  constexpr int BM = 64, BN = 64, BK = 16, LDT = 68;
  __shared__ float As[2][BK][LDT];
  __shared__ float Ws[2][BK][LDT];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int ntn = (p.N + BN - 1) / BN;
  const int m0 = (blockIdx.x / ntn) * BM, n0 = (blockIdx.x % ntn) * BN;

  // K-step list. cin % 16 == 0: a K-step lies inside one tap and the channel range may be restricted to the groups of this
  // workgroup's output columns [c_lo, c_hi); otherwise K is walked linearly and the tap is found per 4-channel vector.
  const int cin = p.cin;
  const bool tapwise = (cin & 15) == 0;
  int c_lo = 0, c_hi = cin;
  if (p.groups > 1) {
    const int g_lo = n0 / p.cpg_out, g_hi = min(p.N - 1, n0 + BN - 1) / p.cpg_out;
    c_lo = (g_lo * p.cpg_in) & ~15;
    c_hi = min(cin, ((g_hi + 1) * p.cpg_in + 15) & ~15);
  }
  const int spt = tapwise ? (c_hi - c_lo) >> 4 : 1;
  const int nsteps = tapwise ? p.ntaps * spt : p.K >> 4;

  // staging assignment: one float4 of A and one of W per thread per K-step
  const int r = tid >> 2, kv = tid & 3;
  int pixb, iy0, ix0;
  {
    const int m = m0 + r;
    if (m < p.M) {
      const int HoWo = p.Ho * p.Wo;
      const int b = m / HoWo, rem = m - b * HoWo;
      const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
      pixb = b * p.H * p.W; iy0 = oy * p.stride; ix0 = ox * p.stride;
    } else { pixb = 0; iy0 = -1000000; ix0 = 0; }
  }
  const int wrow = n0 + r;
  const bool wok = wrow < p.N;
  const float* wbase = p.w + (size_t)(wok ? wrow : 0) * p.K;
  const int shift = p.shift, parity = p.parity;

  float4 ra, rw;
  auto load_tile = [&](int kt) {
    int tap, c, wk;
    bool ev = true;
    if (tapwise) {
      tap = kt / spt;
      c = c_lo + ((kt - tap * spt) << 4) + kv * 4;
      wk = tap * cin + c;
    } else {
      wk = (kt << 4) + kv * 4;
      tap = wk / cin;
      c = wk - tap * cin;
      ev = tap < p.ntaps;
    }
    const int e = p.taptab[ev ? tap : 0];
    const int dx = (e & 63) - 32, dy = ((e >> 6) & 63) - 32;
    const int ly = iy0 + dy, lx = ix0 + dx;
    const int sy = ly >> shift, sx = lx >> shift;
    bool ok = ev && ly >= 0 && lx >= 0 && sy < p.H && sx < p.W;
    if (parity) ok = ok && (((ly | lx) & 1) == 0);
    ra = ok ? *(const float4*)(p.x + (size_t)(pixb + sy * p.W + sx) * p.x_ld + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    rw = wok ? *(const float4*)(wbase + wk) : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto store_tile = [&](int buf) {
    As[buf][kv * 4 + 0][r] = ra.x; As[buf][kv * 4 + 1][r] = ra.y; As[buf][kv * 4 + 2][r] = ra.z; As[buf][kv * 4 + 3][r] = ra.w;
    Ws[buf][kv * 4 + 0][r] = rw.x; Ws[buf][kv * 4 + 1][r] = rw.y; Ws[buf][kv * 4 + 2][r] = rw.z; Ws[buf][kv * 4 + 3][r] = rw.w;
  };

  f32x16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  const int fr = lane & 31, fh = lane >> 5;

  if (nsteps > 0) {
    load_tile(0);
    store_tile(0);
    __syncthreads();
    for (int kt = 0; kt < nsteps; ++kt) {
      const int cur = kt & 1;
      const bool more = kt + 1 < nsteps;
      if (more) load_tile(kt + 1);
#pragma unroll
      for (int kk = 0; kk < BK / 2; ++kk) {
        const float a = Ws[cur][kk * 2 + fh][wn * 32 + fr];
        const float b = As[cur][kk * 2 + fh][wm * 32 + fr];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
      }
      if (more) store_tile(cur ^ 1);
      __syncthreads();
    }
  }

  // epilogue: acc[v] = out[m = m0 + wm*32 + fr][n = n0 + wn*32 + (v>>2)*8 + fh*4 + (v&3)]
  const int m = m0 + wm * 32 + fr;
  if (m >= p.M) return;
  const int flags = p.flags;
#pragma unroll
  for (int vg = 0; vg < 4; ++vg) {
    const int nb = n0 + wn * 32 + vg * 8 + fh * 4;
    if (nb >= p.N) continue;
    float h[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) h[q] = acc[vg * 4 + q];
    const bool full = nb + 4 <= p.N;
    if (flags & CF_BIAS) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (nb + q < p.N) h[q] += p.bias[nb + q];
    }
    if (flags & CF_RES) {
      const float* rp = p.res + (size_t)m * p.res_ld + nb;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (nb + q < p.N) h[q] += rp[q];
    }
    if (flags & CF_RELU) {
#pragma unroll
      for (int q = 0; q < 4; ++q) h[q] = fmaxf(h[q], 0.f);
    }
    if (flags & CF_RELU6) {
#pragma unroll
      for (int q = 0; q < 4; ++q) h[q] = fminf(fmaxf(h[q], 0.f), 6.f);
    }
    if (flags & CF_MASK) {
      const float* mp = p.mask + (size_t)m * p.mask_ld + nb;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (nb + q < p.N && !(mp[q] > 0.f)) h[q] = 0.f;
    }
    float* yp = p.y + (size_t)m * p.y_ld + nb;
    if (full && !(p.y_ld & 3)) {
      *(float4*)yp = make_float4(h[0], h[1], h[2], h[3]);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (nb + q < p.N) yp[q] = h[q];
    }
  }
}

// Narrow outputs (N <= 4: the input gradient of the guide's first convolution -- 3 image channels from 49 taps x 64 channels -- would fill
// 3 of the 64 columns of an MFMA tile): one thread per output pixel, the weights of all N columns through the scalar cache, the SAME
// k-ordered fmaf chain as the MFMA kernel.  A tap that the gather rejects (outside the image, wrong parity of a dilated gather)
// contributes exact zeros there and is skipped here, so the results are bit-identical (tests/test_guide_f32_gpu.py).
__global__ __launch_bounds__(256) void conv_f32_narrow_kernel(ConvF32Params p) {
  const int tid = threadIdx.x;
  const float* __restrict__ wsm = p.w;                // [N][K]: wave-uniform addresses -> scalar loads, the weights are SGPR operands of the fmas
  const int m = blockIdx.x * 256 + tid;
  if (m >= p.M) return;
  const int HoWo = p.Ho * p.Wo;
  const int b = m / HoWo, rem = m - b * HoWo;
  const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
  const int pixb = b * p.H * p.W, iy0 = oy * p.stride, ix0 = ox * p.stride;
  const int shift = p.shift, cin = p.cin, K = p.K, N = p.N;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int tap = 0; tap < p.ntaps; ++tap) {
    const int e = p.taptab[tap];
    const int dx = (e & 63) - 32, dy = ((e >> 6) & 63) - 32;
    const int ly = iy0 + dy, lx = ix0 + dx;
    const int sy = ly >> shift, sx = lx >> shift;
    bool ok = ly >= 0 && lx >= 0 && sy < p.H && sx < p.W;
    if (p.parity) ok = ok && (((ly | lx) & 1) == 0);
    if (!ok) continue;
    const float* xp = p.x + (size_t)(pixb + sy * p.W + sx) * p.x_ld;
    const float* wp = wsm + tap * cin;
    for (int c = 0; c < cin; c += 4) {
      const float4 xv = *(const float4*)(xp + c);
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        if (n < N) {
          const float4 wv = *(const float4*)(wp + n * K + c);
          acc[n] = __builtin_fmaf(wv.x, xv.x, acc[n]);
          acc[n] = __builtin_fmaf(wv.y, xv.y, acc[n]);
          acc[n] = __builtin_fmaf(wv.z, xv.z, acc[n]);
          acc[n] = __builtin_fmaf(wv.w, xv.w, acc[n]);
        }
      }
    }
  }
  const int flags = p.flags;
  for (int n = 0; n < N; ++n) {
    float h = acc[n];
    if (flags & CF_BIAS) h += p.bias[n];
    if (flags & CF_RES) h += p.res[(size_t)m * p.res_ld + n];
    if (flags & CF_RELU) h = fmaxf(h, 0.f);
    if (flags & CF_RELU6) h = fminf(fmaxf(h, 0.f), 6.f);
    if ((flags & CF_MASK) && !(p.mask[(size_t)m * p.mask_ld + n] > 0.f)) h = 0.f;
    p.y[(size_t)m * p.y_ld + n] = h;
  }
}

}  // namespace

hipError_t launch_conv_f32(const ConvF32Params& p, hipStream_t s) {
  if ((p.K & 15) || (p.cin & 3) || (p.x_ld & 3)) return hipErrorInvalidValue;
  if (p.groups > 1 && ((p.cin & 15) || p.cpg_in < 1 || p.cpg_out < 1)) return hipErrorInvalidValue;
  if ((size_t)p.B * p.H * p.W * (size_t)p.x_ld >= 0x7FFF0000ull) return hipErrorInvalidValue;
  if (p.M <= 0 || p.N <= 0) return hipSuccess;
  static const int narrow = getenv("DD_F32_NARROW") ? atoi(getenv("DD_F32_NARROW")) : 1;
  if (narrow && p.N <= 4 && p.groups <= 1 && (size_t)p.N * p.K * 4 <= 65536 && p.M >= 4096) {
    hipLaunchKernelGGL(conv_f32_narrow_kernel, dim3((p.M + 255) / 256), dim3(256), 0, s, p);
    return hipGetLastError();
  }
  const int ntm = (p.M + 63) / 64, ntn = (p.N + 63) / 64;
  hipLaunchKernelGGL(conv_f32_kernel, dim3(ntm * ntn), dim3(256), 0, s, p);
  return hipGetLastError();
}
