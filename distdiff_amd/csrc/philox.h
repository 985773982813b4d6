// The counter-based generator's device functions (gfx950), shared by rng.hip (the noise tensors and the fused add_noise) and
// sampler_step.hip (the step noise of eta > 0, generated in registers): Philox4x32-10 and the Box-Muller of its word pairs.
// Every body carries `#pragma clang fp contract(off)`: each product and sum is rounded on its own whichever file includes this header
// and whatever -ffp-contract that file is built with, because the values generated inside a kernel have to be the bits of the tensors
// dd_randn_units writes.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, unsigned k0, unsigned k1) {
#pragma clang fp contract(off)
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c.x, p1 = 0xCD9E8D57ull * c.z;
    c = make_uint4((unsigned)(p1 >> 32) ^ c.y ^ k0, (unsigned)p1, (unsigned)(p0 >> 32) ^ c.w ^ k1, (unsigned)p0);
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c;
}

// u1 = (wa + 0.5) 2^-32 in (0,1), u2 = (wb + 0.5) 2^-32.  In the upper half u1 would round to 1 in fp32 and lose the small radii:
// ln u1 = log1p(-(1 - u1)) there, with 1 - u1 = (~wa + 0.5) 2^-32 exact to one rounding.  Library logf / log1pf / sincospif (a few
// ulp), not the fast intrinsics: the tails are what this generator is for.  logf and sqrtf are spelled as the builtins the HIP headers
// forward them to: a header's forwarding function is compiled under the including file's -ffp-contract, not under the pragma below, and
// the `contract` flag it would leave on the call changes how the backend expands the logarithm (measured: other last bits).
__device__ __forceinline__ void box_muller(unsigned wa, unsigned wb, float& n0, float& n1) {
#pragma clang fp contract(off)
  const float l = (wa & 0x80000000u) ? log1pf(-(((float)(~wa) + 0.5f) * 0x1p-32f)) : __builtin_logf(((float)wa + 0.5f) * 0x1p-32f);
  const float r = __builtin_sqrtf(-2.f * l);
  float sn, cs;
  sincospif(((float)wb + 0.5f) * 0x1p-31f, &sn, &cs);
  n0 = r * cs;
  n1 = r * sn;
}

// the four values of block q of (stream, unit id): U[0,1) for stream 2 (e), N(0,1) for every other
__device__ __forceinline__ void block_values(unsigned q, int rng_stream, unsigned id_lo, unsigned id_hi, unsigned k0, unsigned k1, float v[4]) {
#pragma clang fp contract(off)
  const uint4 w = philox4x32_10(make_uint4(q, (unsigned)rng_stream, id_lo, id_hi), k0, k1);
  if (rng_stream == 2) {
    v[0] = (float)(w.x >> 8) * 0x1p-24f; v[1] = (float)(w.y >> 8) * 0x1p-24f;
    v[2] = (float)(w.z >> 8) * 0x1p-24f; v[3] = (float)(w.w >> 8) * 0x1p-24f;
  } else {
    box_muller(w.x, w.y, v[0], v[1]);
    box_muller(w.z, w.w, v[2], v[3]);
  }
}
