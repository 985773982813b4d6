// The sampler step (gfx950): classifier-free-guidance mix, optional CFG rescale (Lin et al. 2023; diffusers rescale_noise_cfg), the
// scheduler update (diffusers DDIMScheduler.step, eta in [0, 1]; DPMSolverMultistepScheduler: dpmsolver++, order 2, midpoint) and its VJP.
// One forward kernel template, one backward kernel template, one launcher each; the modes are listed at StepParams in kernels.h.
//
//   m  = u + s (c - u),  m^ = k_b m  (k_b = phi sigma_c / sigma_m + 1 - phi per image; 1 without rescale)
//   x0 = A_z z + A_m m^,  z' = B_z z + B_m m^ [+ c2m (x0 - x0_prev)] [+ sigma n]      (both brackets: SDE-DPM-Solver++(2M))
//
// One thread per pixel: both CFG halves of the 8-wide fp32 NHWC row come in as 16-byte loads, the NCHW reads and writes are coalesced
// along the pixels.  grid = (ceil(HW / 256), B).  No atomics: bitwise deterministic.
//
// ROUNDING.  The per-element arithmetic of both kernels is compiled with contraction off and spells every fused multiply-add as
// __builtin_fmaf, so which results are rounded once and which twice is a statement of this file.  Each form is the one the kernel
// that first served that mode happened to compile to (the former kernel is named at the line); tests/test_sampler_step_bits_gpu.py
// holds their bits.  Do not "simplify" a * b + c * d into an fma or the reverse: it changes the latents of every image.
// The noise term of eta > 0 is zp = (b0 * t + b1 * m) + sigma * n: the no-history expression on the eta tables, then the product rounded,
// then the sum rounded, no fma -- what torch gives for z'(noise = 0) + sigma * n in fp32 (tests/test_ddim_eta_gpu.py).
// With a history and noise (SDE-DPM-Solver++(2M), on the SDE rows) it is zp = (fmaf(b0, t, b1 * m) + c2m * (x - xp)) + sigma * n: the HIST
// expression, then the product rounded, then the sum rounded, no fma -- z' of the HIST kernel on the same rows and c, + sigma * n by torch
// in fp32 (tests/test_dpm_sde_gpu.py).  The six instantiations without that pair are untouched by it.
#include <cmath>

#include "common.h"
#include "kernels.h"
#include "philox.h"

namespace {

#define STEP_THREADS 256
__device__ __forceinline__ void load_row8(const float* p, int C, float* v) {
  const float4 a = *(const float4*)p;
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = v[5] = v[6] = v[7] = 0.f;
  if (C > 4) { const float4 b = *(const float4*)(p + 4); v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w; }
}

// EPS: (epsilon, no rescale) in the division form on the five-float row coef = {s, sqrt a, sqrt(1-a), sqrt a', sqrt(1-a')}:
//   x0 = (z - sqrt(1-a) m) / sqrt a,  z' = sqrt a' x0 + sqrt(1-a') m
// otherwise the linear form on lin = {A_z, A_m, B_z, B_m} (sampler_step_coefs).  HIST adds c2m (x0 - x0_prev) and always writes x0,
// which may alias x0_prev: each thread reads its own element before it writes it.  NOISE adds sigma n on the stochastic rows (eta or SDE)
// of coef / lin and steps rows rng_row0 + blockIdx.y: n is read from p.noise, or is lane j & 3 of Philox block j >> 2 of the row's unit,
// j = ch * HW + pix -- one thread per pixel as before, so each thread computes the block of each of its elements (and its neighbours
// compute it again: 4x the Philox work of rng.hip, microseconds against the UNet) and the Box-Muller of the one word pair it needs.
// HIST with NOISE keeps the row ranges of the generated form (DD_RNG_UNITS ids per launch): a launch reads and writes the elements of
// its own rows only -- z, x0_prev, x0, z_prev alike -- so x0 == x0_prev stays legal across the launches of one batch.
// HALVES == 1 (StepParams::halves, the CFG-free engine): m2 holds the conditional rows alone and m = c -- the unconditional row and
// coef[0] are not read, the mix is not evaluated; everything after `mix` is the same text.  fmaf(s, c - c, c) == c for finite c, so this
// is the two-half kernel on m2 = [c; c] bit for bit (tests/test_cfg_free_gpu.py).
template <bool EPS, bool HIST, bool NOISE, int HALVES>
__global__ __launch_bounds__(STEP_THREADS) void sampler_step_kernel(const StepParams p) {
#pragma clang fp contract(off)
  const int b = NOISE ? p.rng_row0 + blockIdx.y : blockIdx.y, pix = blockIdx.x * STEP_THREADS + threadIdx.x;
  if (pix >= p.HW) return;
  const float s = HALVES == 2 ? p.coef[0] : 1.f;
  // EPS: {sqrt a, sqrt(1-a)} and {sqrt a', sqrt(1-a')}, the latter on (x0, m); linear: {A_z, A_m} and {B_z, B_m}, on (z, m^)
  const float a0 = EPS ? p.coef[1] : p.lin[0], a1 = EPS ? p.coef[2] : p.lin[1];
  const float b0 = EPS ? p.coef[3] : p.lin[2], b1 = EPS ? p.coef[4] : p.lin[3];
  const float k = HALVES == 2 && !EPS && p.phi != 0.f ? p.stats[b * 8] : 1.f;
  float u[8], c[8];
  if (HALVES == 2) load_row8(p.m2 + ((size_t)b * p.HW + pix) * p.ld, p.C, u);
  load_row8(p.m2 + ((size_t)(HALVES == 2 ? p.B + b : b) * p.HW + pix) * p.ld, p.C, c);
#pragma unroll
  for (int ch = 0; ch < 8; ++ch) {
    if (ch < p.C) {
      const size_t zi = ((size_t)b * p.C + ch) * p.HW + pix;
      const float zz = p.z[zi], xp = HIST ? p.x0_prev[zi] : 0.f;
      const float mix = HALVES == 2 ? __builtin_fmaf(s, c[ch] - u[ch], u[ch]) : c[ch];
      const float m = EPS ? mix : k * mix;
      // x0.  EPS: an fma and a correctly rounded division (bits of the former cfg_ddim_kernel); linear: both products rounded, then
      // added (bits of the former linear-form sampler_step_kernel) -- with and without a history
      const float x = EPS ? __builtin_fmaf(-a1, m, zz) / a0 : a0 * zz + a1 * m;
      const float t = EPS ? x : zz;
      float zp;
      // z'.  With a history one fma, then the separately rounded c2m (x0 - x0_prev) added (bits of the former sampler_step_2m_kernel,
      // both instantiations); without, both products rounded, then added (cfg_ddim_kernel and sampler_step_kernel)
      if (HIST) zp = __builtin_fmaf(b0, t, b1 * m) + p.c2m * (x - xp);
      else zp = b0 * t + b1 * m;
      if (NOISE) {
        float n;
        if (p.noise) {
          n = p.noise[zi];
        } else {
          const unsigned j = (unsigned)ch * (unsigned)p.HW + (unsigned)pix;
          const uint4 w = philox4x32_10(make_uint4(j >> 2, (unsigned)p.rng_stream, p.rng_ids.lo[blockIdx.y], p.rng_ids.hi[blockIdx.y]),
                                        (unsigned)p.rng_seed, (unsigned)(p.rng_seed >> 32));
          float n0, n1;
          box_muller((j & 2) ? w.z : w.x, (j & 2) ? w.w : w.y, n0, n1);
          n = (j & 1) ? n1 : n0;
        }
        zp = zp + p.sigma * n;
      }
      if (HIST || p.x0) p.x0[zi] = x;
      p.z_prev[zi] = zp;
    }
  }
}

__device__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
  return t;
}

// CFG rescale statistics, stage 1: per (image, 256-pixel block) the count, mean and centred second moment of c and of m over the C real
// columns.  part[(b * nblk + blk) * 8] = {n, mean_c, M2_c, mean_m, M2_m}.  Fixed reduction order: bitwise deterministic.
__global__ __launch_bounds__(STEP_THREADS) void cfg_stats_part_kernel(const float* m2, int ld, int B, int C, int HW, const float* coef,
                                                                      float* part) {
  __shared__ float red[8];
  const int b = blockIdx.y, pix = blockIdx.x * STEP_THREADS + threadIdx.x;
  const bool valid = pix < HW;
  const float s = coef[0];
  float c[8], m[8];
  float sc = 0.f, sm = 0.f;
  if (valid) {
    float u[8];
    load_row8(m2 + ((size_t)b * HW + pix) * ld, C, u);
    load_row8(m2 + ((size_t)(B + b) * HW + pix) * ld, C, c);
#pragma unroll
    for (int ch = 0; ch < 8; ++ch)
      if (ch < C) { m[ch] = u[ch] + s * (c[ch] - u[ch]); sc += c[ch]; sm += m[ch]; }
  }
  const float n = (float)(min(STEP_THREADS, HW - (int)blockIdx.x * STEP_THREADS) * C);
  const float mean_c = block_sum(sc, red) / n, mean_m = block_sum(sm, red) / n;
  float qc = 0.f, qm = 0.f;
  if (valid) {
#pragma unroll
    for (int ch = 0; ch < 8; ++ch)
      if (ch < C) { const float dc = c[ch] - mean_c, dm = m[ch] - mean_m; qc += dc * dc; qm += dm * dm; }
  }
  const float M2c = block_sum(qc, red), M2m = block_sum(qm, red);
  if (threadIdx.x == 0) {
    float* o = part + ((size_t)b * gridDim.x + blockIdx.x) * 8;
    o[0] = n; o[1] = mean_c; o[2] = M2c; o[3] = mean_m; o[4] = M2m;
  }
}

// stage 2: one thread per image merges the block partials in block order (counts, means, M2: Chan et al., as gn_finalize_chan_kernel
// does) and writes stats[b * 8] = {k, sigma_c, sigma_m, mean_c, mean_m, N, phi}: sigma unbiased (N - 1), k = phi sigma_c / sigma_m + 1 - phi
__global__ void cfg_stats_final_kernel(const float* part, int nblk, int B, float phi, float* stats) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double n = 0, mc = 0, Mc = 0, mm = 0, Mm = 0;
  for (int i = 0; i < nblk; ++i) {
    const float* p = part + ((size_t)b * nblk + i) * 8;
    const double nb = p[0], t = n + nb, dc = (double)p[1] - mc, dm = (double)p[3] - mm;
    Mc += (double)p[2] + dc * dc * n * nb / t; mc += dc * nb / t;
    Mm += (double)p[4] + dm * dm * n * nb / t; mm += dm * nb / t;
    n = t;
  }
  const double sig_c = sqrt(Mc / (n - 1)), sig_m = sqrt(Mm / (n - 1));
  float* o = stats + (size_t)b * 8;
  o[0] = (float)((double)phi * sig_c / sig_m + 1.0 - (double)phi);
  o[1] = (float)sig_c; o[2] = (float)sig_m; o[3] = (float)mc; o[4] = (float)mm; o[5] = (float)n; o[6] = phi; o[7] = 0.f;
}

// backward, rescale only: per-block partial of sum(g^ m) with g^ = A_m g_x0 + B_m g_z' the gradient on m^
__global__ __launch_bounds__(STEP_THREADS) void sampler_step_bwd_dot_kernel(const float* g_x0, const float* g_zprev, const float* m2, int ld,
                                                                            int B, int C, int HW, const float* coef, const float* lin,
                                                                            float* dpart) {
  __shared__ float red[8];
  const int b = blockIdx.y, pix = blockIdx.x * STEP_THREADS + threadIdx.x;
  const float s = coef[0], Am = lin[1], Bm = lin[3];
  float acc = 0.f;
  if (pix < HW) {
    float u[8], c[8];
    load_row8(m2 + ((size_t)b * HW + pix) * ld, C, u);
    load_row8(m2 + ((size_t)(B + b) * HW + pix) * ld, C, c);
#pragma unroll
    for (int ch = 0; ch < 8; ++ch)
      if (ch < C) {
        const size_t zi = ((size_t)b * C + ch) * HW + pix;
        const float gh = Am * (g_x0 ? g_x0[zi] : 0.f) + Bm * (g_zprev ? g_zprev[zi] : 0.f);
        acc += gh * (u[ch] + s * (c[ch] - u[ch]));
      }
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) dpart[(size_t)b * gridDim.x + blockIdx.x] = acc;
}

// VJP of the step in x0 and z' (the history term is not differentiated: the guidance calls differentiate x0, which does not depend on
// it): g_z (NCHW fp32) and g_m2, bf16 NHWC rows (all ld columns written, padding = 0), g_m split (1 - s, s) onto the CFG halves.
//   EPS:      h = g_x0 + sqrt a' g_z',  g_m = (-sqrt(1-a) / sqrt a) h + sqrt(1-a') g_z',  g_z = h / sqrt a
//   linear:   g_z = A_z g_x0 + B_z g_z',  g^ = A_m g_x0 + B_m g_z'; with rescale (p.m2 = the model output of that step, p.part from
//             the kernel above, S its sum over the image):
//             g_m = k g^ - phi sigma_c / sigma_m^2 . S (m - mean_m) / ((N - 1) sigma_m),  g_c += phi / sigma_m . S (c - mean_c) / ((N - 1) sigma_c)
// HALVES == 1: g_m itself goes to rows [B*HW, ld] of g_m2 -- no (1 - s, s) split, coef[0] is not read, no rescale (refused by the launcher).
// It is the conditional row of the two-half kernel at s = 1 bit for bit: 1 * g_m and fmaf(1, g_m, 0) are g_m.
template <bool EPS, int HALVES>
__global__ __launch_bounds__(STEP_THREADS) void sampler_step_bwd_kernel(const StepParams p, const float* g_x0, const float* g_zprev,
                                                                        bf16_t* g_m2, float* g_z) {
#pragma clang fp contract(off)
  __shared__ float S_sh;
  const bool rescale = HALVES == 2 && !EPS && p.phi != 0.f;
  const int b = blockIdx.y, pix = blockIdx.x * STEP_THREADS + threadIdx.x;
  float k = 1.f, tm = 0.f, tc = 0.f, mean_c = 0.f, mean_m = 0.f;
  if (rescale) {
    if (threadIdx.x == 0) {
      double S = 0;
      for (int i = 0; i < (int)gridDim.x; ++i) S += (double)p.part[(size_t)b * gridDim.x + i];     // block order: deterministic
      S_sh = (float)S;
    }
    __syncthreads();
    const float* st = p.stats + (size_t)b * 8;
    const float sig_c = st[1], sig_m = st[2], N1 = st[5] - 1.f, phi = st[6];
    k = st[0]; mean_c = st[3]; mean_m = st[4];
    tm = phi * sig_c / (sig_m * sig_m) * S_sh / (N1 * sig_m);
    tc = phi / sig_m * S_sh / (N1 * sig_c);
  }
  if (pix >= p.HW) return;
  const float s = HALVES == 2 ? p.coef[0] : 1.f;
  // EPS: {sqrt a, sqrt(1-a)} and {sqrt a', sqrt(1-a')}; linear: {A_z, A_m} and {B_z, B_m}
  const float a0 = EPS ? p.coef[1] : p.lin[0], a1 = EPS ? p.coef[2] : p.lin[1];
  const float b0 = EPS ? p.coef[3] : p.lin[2], b1 = EPS ? p.coef[4] : p.lin[3];
  float u[8], c[8];
  if (rescale) {
    load_row8(p.m2 + ((size_t)b * p.HW + pix) * p.ld, p.C, u);
    load_row8(p.m2 + ((size_t)(p.B + b) * p.HW + pix) * p.ld, p.C, c);
  }
  float gu[8], gc[8];
#pragma unroll
  for (int ch = 0; ch < 8; ++ch) {
    gu[ch] = 0.f; gc[ch] = 0.f;
    if (ch < p.C) {
      const size_t zi = ((size_t)b * p.C + ch) * p.HW + pix;
      const float gx = g_x0 ? g_x0[zi] : 0.f, gp = g_zprev ? g_zprev[zi] : 0.f;
      float gm;
      if (EPS) {   // bits of the former cfg_ddim_bwd_kernel: h fused, g_m the sum of two rounded products, plain s g_m
        const float h = __builtin_fmaf(b0, gp, gx);
        g_z[zi] = h / a0;
        gm = -a1 / a0 * h + b1 * gp;
        gc[ch] = HALVES == 2 ? s * gm : gm;
      } else {     // bits of the former linear-form backward: g_z the sum of two rounded products, g^ and s g_m + extra fused
        g_z[zi] = a0 * gx + b0 * gp;
        gm = __builtin_fmaf(a1, gx, b1 * gp);
        float extra = 0.f;
        if (rescale) {
          const float m = __builtin_fmaf(s, c[ch] - u[ch], u[ch]);
          gm = k * gm - tm * (m - mean_m);
          extra = tc * (c[ch] - mean_c);
        }
        gc[ch] = HALVES == 2 ? __builtin_fmaf(s, gm, extra) : gm;
      }
      gu[ch] = (1.f - s) * gm;
    }
  }
  const uint4 zero = make_uint4(0, 0, 0, 0);
  if (HALVES == 1) {
    bf16_t* rc = g_m2 + ((size_t)b * p.HW + pix) * p.ld;
    *(uint4*)rc = pack8(gc);
    for (int c0 = 8; c0 < p.ld; c0 += 8) *(uint4*)(rc + c0) = zero;
    return;
  }
  bf16_t* ru = g_m2 + ((size_t)b * p.HW + pix) * p.ld;
  bf16_t* rc = g_m2 + ((size_t)(p.B + b) * p.HW + pix) * p.ld;
  *(uint4*)ru = pack8(gu); *(uint4*)rc = pack8(gc);
  for (int c0 = 8; c0 < p.ld; c0 += 8) { *(uint4*)(ru + c0) = zero; *(uint4*)(rc + c0) = zero; }
}

// what both launchers refuse in front of any launch.  The 16-byte row accesses need ld % 8 == 0, the thread map C <= 8, the grid B <= 65535
// One half (CFG-free) has no rescale: its factor is identically 1 at m = c and the statistics pass is not built for one half
bool step_args_ok(const StepParams& p, bool eps) {
  const bool shape_ok = p.B >= 1 && p.B <= 65535 && p.C >= 1 && p.C <= 8 && p.HW >= 1 && p.ld >= 8 && !(p.ld & 7);
  const bool halves_ok = p.halves == 2 || (p.halves == 1 && p.phi == 0.f);
  return shape_ok && halves_ok && p.prediction_type >= 0 && p.prediction_type <= 2 && (eps || p.lin) && (p.phi == 0.f || (p.stats && p.part));
}
// the forward instantiation of one launch
template <int HALVES>
auto step_kernel(bool eps, bool hist, bool noise) -> void (*)(StepParams) {
  if (noise)
    return eps ? (hist ? sampler_step_kernel<true, true, true, HALVES> : sampler_step_kernel<true, false, true, HALVES>)
               : (hist ? sampler_step_kernel<false, true, true, HALVES> : sampler_step_kernel<false, false, true, HALVES>);
  return eps ? (hist ? sampler_step_kernel<true, true, false, HALVES> : sampler_step_kernel<true, false, false, HALVES>)
             : (hist ? sampler_step_kernel<false, true, false, HALVES> : sampler_step_kernel<false, false, false, HALVES>);
}

}  // namespace

// the four step coefficients in double (B_m = sqrt(1-a') sqrt(a) - sqrt(a') sqrt(1-a) cancels here and not in fp32); the v-prediction
// form never divides by sqrt(a): a zero-terminal-SNR table has a = 0 exactly at its first trailing step
static int step_coefs_d(int prediction_type, double a, double ap, double sbp, float* out4) {
  const double sa = sqrt(a), sb = sqrt(1 - a), sap = sqrt(ap);
  double Az, Am, Bz, Bm;
  if (prediction_type == 0) {
    if (!(a > 0)) return -1;
    Az = 1 / sa; Am = -sb / sa; Bz = sap / sa; Bm = sbp - sap * sb / sa;
  } else if (prediction_type == 1) {
    Az = sa; Am = -sb; Bz = sap * sa + sbp * sb; Bm = sbp * sa - sap * sb;
  } else if (prediction_type == 2) {
    if (!(a < 1)) return -1;
    Az = 0; Am = 1; Bz = sbp / sb; Bm = sap - sbp * sa / sb;
  } else {
    return -1;
  }
  out4[0] = (float)Az; out4[1] = (float)Am; out4[2] = (float)Bz; out4[3] = (float)Bm;
  return 0;
}
// eta in [0, 1]: the direction term keeps d = sqrt(max(0, 1 - a' - sigma^2)) of the noise level 1 - a' and sigma^2 goes to fresh noise.
// The max is needed: at a = 0 (the first trailing step of a zero-terminal-SNR table) eta = 1 gives 1 - a' - sigma^2 ~ 1e-16 of either
// sign.  eta = 0 takes sigma = 0 without evaluating the variance: d is then sqrt(1 - a') and the floats are those of rule 0.
static void eta_sigma_d(double a, double ap, double eta, double* sigma, double* d) {
  *sigma = eta > 0 ? eta * sqrt((1 - ap) / (1 - a) * (1 - a / ap)) : 0.0;
  const double d2 = 1 - ap - *sigma * *sigma;
  *d = sqrt(d2 > 0 ? d2 : 0.0);
}
// SDE-DPM-Solver++(2M), s in [0, 1] (k-diffusion sample_dpmpp_2m_sde's eta): with h = lambda(a') - lambda(a) the direction term keeps
// d = sqrt(1-a') e^(-s h) and sigma_n = sqrt(1-a') sqrt(-expm1(-2 s h)) goes to fresh noise, d^2 + sigma_n^2 = 1 - a'.  The limits are
// taken here, never computed: s = 0 and h <= 0 (a' = a) give (sqrt(1-a'), 0) -- the floats of rule 0 --, a' = 1 gives (0, 0),
// a = 0 (h = +inf: the first trailing step of a zero-terminal-SNR table) gives (0, sqrt(1-a')).
static void sde_sigma_d(double a, double ap, double s, double* sigma, double* d) {
  const double sbp = sqrt(1 - ap);
  *sigma = 0.0; *d = sbp;
  if (!(s > 0) || !(ap < 1)) return;
  if (!(a > 0)) { *sigma = sbp; *d = 0.0; return; }
  const double h = 0.5 * (log(ap / (1 - ap)) - log(a / (1 - a)));
  if (!(h > 0)) return;
  if (!std::isfinite(h)) { *sigma = sbp; *d = 0.0; return; }
  *d = sbp * exp(-s * h);
  *sigma = sbp * sqrt(-expm1(-2 * s * h));
}
size_t sampler_step_scratch_floats(int B, int HW) { return (size_t)B * ((HW + STEP_THREADS - 1) / STEP_THREADS) * 8; }

// c_i of the second-order step i of an n-step schedule, from alphas_cumprod at step i - 1, at step i and at its previous timestep.
// With lambda(a) = ln(a / (1 - a)) / 2, h = lambda(a') - lambda(a) and r = (lambda(a) - lambda(a_before)) / h:
//   c = sqrt(a') (1 - e^-h) / (2 r)
// Exactly 0 -- the step is then the first-order one -- for the first and the last step of the schedule and wherever a lambda is not
// finite (a = 0 of a zero-terminal-SNR table, a' = 1) or c itself is not: never NaN or inf.
// The SDE variant with s in [0, 1] has c = sqrt(a') (1 - e^-((1+s) h)) / (2 r), the same zeros, and at s = 0 the same double expression.
static float coef_2m_s(int i, int n, double a_before, double a, double ap, double s) {
  if (i <= 0 || i >= n - 1) return 0.f;
  const double l0 = 0.5 * log(a_before / (1 - a_before)), l1 = 0.5 * log(a / (1 - a)), l2 = 0.5 * log(ap / (1 - ap));
  if (!std::isfinite(l0) || !std::isfinite(l1) || !std::isfinite(l2)) return 0.f;
  const double h = l2 - l1, r = (l1 - l0) / h;
  const double c = sqrt(ap) * -expm1(s > 0 ? -(1 + s) * h : -h) / (2 * r);
  return std::isfinite(c) && std::isfinite((float)c) ? (float)c : 0.f;
}
// the row of one step under one rule (kernels.h).  The order is part of the contract: the range of s, then (sigma, d) of the rule, then
// the type and the singular steps inside step_coefs_d, and only then the first write to *out
int sampler_step_row(const StepRule& r, int i, int n, double a_before, double a, double ap, StepRow* out) {
  if (r.noise < 0 || r.noise > 2 || (r.noise && !(r.s >= 0 && r.s <= 1))) return -1;
  double sigma = 0.0, d = sqrt(1 - ap);
  if (r.noise == 1) eta_sigma_d(a, ap, r.s, &sigma, &d);
  if (r.noise == 2) sde_sigma_d(a, ap, r.s, &sigma, &d);
  if (step_coefs_d(r.prediction_type, a, ap, d, out->lin)) return -1;
  out->d = (float)d; out->sigma = (float)sigma;
  out->c2m = coef_2m_s(i, n, a_before, a, ap, r.noise == 2 ? r.s : 0.0);
  // the deterministic rule does not look (a = 1e-80 gives an infinite row with 0): a schedule that refused it would be another schedule
  if (r.noise)
    for (const float v : {out->lin[0], out->lin[1], out->lin[2], out->lin[3], out->sigma})
      if (!std::isfinite(v)) return -2;
  return 0;
}

hipError_t launch_sampler_step(const StepParams& p, hipStream_t s) {
  const bool eps = p.prediction_type == 0 && p.phi == 0.f;
  const bool hist = p.x0_prev && p.c2m != 0.f;              // otherwise the first-order step: the history is not read
  if (!step_args_ok(p, eps) || (hist && (!p.x0 || !std::isfinite(p.c2m)))) return hipErrorInvalidValue;
  // a stochastic step (eta > 0 or SDE): sigma != 0 and a noise source, the tensor or (rng_count > 0) the generator on rows [rng_row0, rng_row0 + rng_count)
  if (!std::isfinite(p.sigma) || p.rng_count < 0 || p.rng_count > DD_RNG_UNITS) return hipErrorInvalidValue;
  const bool noise = p.sigma != 0.f && (p.noise || p.rng_count > 0), generated = noise && !p.noise;
  // the kernel draws normals: stream 2 (e) is uniform in launch_philox_units and would not be its tensor here
  if (generated && (p.rng_row0 < 0 || p.rng_row0 + p.rng_count > p.B || !rng_stream_ok(p.rng_stream) || p.rng_stream == 2)) return hipErrorInvalidValue;
  const dim3 grid((p.HW + STEP_THREADS - 1) / STEP_THREADS, p.B);
  if (p.phi != 0.f && !(generated && p.rng_row0 > 0)) {     // the statistics of the whole batch, once: with the first row range
    hipLaunchKernelGGL(cfg_stats_part_kernel, grid, dim3(STEP_THREADS), 0, s, p.m2, p.ld, p.B, p.C, p.HW, p.coef, p.part);
    hipLaunchKernelGGL(cfg_stats_final_kernel, dim3((p.B + 63) / 64), dim3(64), 0, s, (const float*)p.part, (int)grid.x, p.B, p.phi, p.stats);
  }
  if (noise) {
    StepParams q = p;
    if (!generated) q.rng_row0 = 0;
    const dim3 rows(grid.x, generated ? p.rng_count : p.B);
    const auto noisy = p.halves == 1 ? step_kernel<1>(eps, hist, true) : step_kernel<2>(eps, hist, true);
    hipLaunchKernelGGL(noisy, rows, dim3(STEP_THREADS), 0, s, q);
    return hipGetLastError();
  }
  const auto kernel = p.halves == 1 ? step_kernel<1>(eps, hist, false) : step_kernel<2>(eps, hist, false);
  hipLaunchKernelGGL(kernel, grid, dim3(STEP_THREADS), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_sampler_step_units(const StepParams& p, const uint64_t* unit_ids, hipStream_t s) {
  if (p.sigma == 0.f || p.noise) return launch_sampler_step(p, s);
  if (!unit_ids) return hipErrorInvalidValue;
  return for_rng_unit_ranges(unit_ids, p.B, [&](const RngUnits& ids, int r0, int cnt) {
    StepParams q = p;
    q.rng_ids = ids; q.rng_row0 = r0; q.rng_count = cnt;
    return launch_sampler_step(q, s);
  });
}

hipError_t launch_sampler_step_bwd(const StepParams& p, const float* g_x0, const float* g_zprev, bf16_t* g_m2, float* g_z, hipStream_t s) {
  const bool eps = p.prediction_type == 0 && p.phi == 0.f;
  if (!step_args_ok(p, eps) || (p.phi != 0.f && !p.m2)) return hipErrorInvalidValue;
  const dim3 grid((p.HW + STEP_THREADS - 1) / STEP_THREADS, p.B);
  if (p.phi != 0.f)
    hipLaunchKernelGGL(sampler_step_bwd_dot_kernel, grid, dim3(STEP_THREADS), 0, s, g_x0, g_zprev, p.m2, p.ld, p.B, p.C, p.HW, p.coef, p.lin, p.part);
  const auto kernel = p.halves == 1 ? (eps ? sampler_step_bwd_kernel<true, 1> : sampler_step_bwd_kernel<false, 1>)
                                    : (eps ? sampler_step_bwd_kernel<true, 2> : sampler_step_bwd_kernel<false, 2>);
  hipLaunchKernelGGL(kernel, grid, dim3(STEP_THREADS), 0, s, p, g_x0, g_zprev, g_m2, g_z);
  return hipGetLastError();
}
