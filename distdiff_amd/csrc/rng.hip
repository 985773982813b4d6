// Counter-based device noise (gfx950): Philox4x32-10 keyed by the run's seed and counted by (element, stream, unit id), so the noise
// of a unit (train image, expand index) depends on nothing else -- not on the row of the batch, the batch size, the grid or the call.
//   key     = (seed lo, seed hi)
//   counter = (j / 4, stream, unit id lo, unit id hi) for element j of the unit's tensor: one 128-bit block per 4 outputs
//   streams : 0 initial noise [C,L,L], 1 offset noise [C], 3 b [4] -- N(0,1);  2 e [4] -- U[0,1);  16 + i the noise of step i of the
//             schedule under eta > 0 [C,L,L] -- N(0,1) (sampler_step.hip generates the same values in registers); 4-15 reserved
// Normals by Box-Muller from the word pairs (w0,w1) and (w2,w3); uniforms (w >> 8) * 2^-24.
// This file is built with -ffp-contract=off (build.py): every product and sum below is rounded on its own, because the fused first op
// of the loop has to give the bits of the two-kernel path (dd_randn_units, then add_noise) that the parity tests cover.
#include "common.h"
#include "kernels.h"
#include "philox.h"

namespace {

// FUSED = false: out[u, j] = value j of unit u in `rng_stream`.
// FUSED = true : out[u, j] = sa * x[u, j] + sb * (n_j + 0.1 * o_c), n from stream 0, o_c from stream 1 at channel c = j / HW when
//                offset_noise -- add_noise (generate_data.py:1164-1176) written from the generated values, no noise tensor in memory.
// One thread per Philox block = 4 consecutive outputs, one 16-byte store when the rows are 16-byte aligned (n % 4 == 0).
template <bool FUSED>
__global__ void philox_units_kernel(RngUnits ids, unsigned k0, unsigned k1, int rng_stream, long long n, float* __restrict__ out,
                                    const float* __restrict__ x, const float* __restrict__ coef, int HW, int offset_noise) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long j0 = q * 4;
  if (j0 >= n) return;
  const int u = blockIdx.y;
  const unsigned id_lo = ids.lo[u], id_hi = ids.hi[u];
  float v[4];
  block_values((unsigned)q, FUSED ? 0 : rng_stream, id_lo, id_hi, k0, k1, v);
  const size_t base = (size_t)u * (size_t)n + (size_t)j0;
  const int cnt = n - j0 < 4 ? (int)(n - j0) : 4;
  if (FUSED) {
    const float sa = coef[0], sb = coef[1];
    int c_have = -1;
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k >= cnt) break;
      float nz = v[k];
      if (offset_noise) {
        const int c = (int)((j0 + k) / HW);
        if ((c >> 2) != c_have) { c_have = c >> 2; block_values((unsigned)c_have, 1, id_lo, id_hi, k0, k1, o); }
        nz = nz + 0.1f * o[c & 3];
      }
      v[k] = sa * x[base + k] + sb * nz;     // two products, one sum, each rounded: what add_noise's own kernel compiles to (elementwise.hip)
    }
  }
  if (cnt == 4 && (n & 3) == 0) {
    *reinterpret_cast<float4*>(out + base) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int k = 0; k < cnt; ++k) out[base + k] = v[k];
  }
}

hipError_t launch(bool fused, const RngUnits& ids, int count, uint64_t seed, int rng_stream, int64_t n, float* out, const float* x,
                  const float* coef, int HW, int offset_noise, hipStream_t s) {
  if (count < 1 || count > DD_RNG_UNITS || n < 1 || !rng_stream_ok(rng_stream)) return hipErrorInvalidValue;
  const long long nq = (n + 3) / 4;
  const dim3 grid((unsigned)((nq + 255) / 256), (unsigned)count);
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
  if (fused) hipLaunchKernelGGL(philox_units_kernel<true>, grid, dim3(256), 0, s, ids, k0, k1, 0, (long long)n, out, x, coef, HW, offset_noise);
  else hipLaunchKernelGGL(philox_units_kernel<false>, grid, dim3(256), 0, s, ids, k0, k1, rng_stream, (long long)n, out, nullptr, nullptr, 1, 0);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_philox_units(const RngUnits& ids, int count, uint64_t seed, int rng_stream, int64_t n_per_unit, float* out, hipStream_t s) {
  return launch(false, ids, count, seed, rng_stream, n_per_unit, out, nullptr, nullptr, 1, 0, s);
}
hipError_t launch_philox_add_noise(const RngUnits& ids, int count, uint64_t seed, const float* x, float* out, int C, int HW, int offset_noise,
                                   const float* coef_dev, hipStream_t s) {
  if (C < 1 || HW < 1) return hipErrorInvalidValue;
  return launch(true, ids, count, seed, 0, (int64_t)C * HW, out, x, coef_dev, HW, offset_noise, s);
}
