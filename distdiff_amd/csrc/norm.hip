// K3/K4 — GroupNorm(+SiLU) and LayerNorm forward/backward on NHWC bf16 rows (gfx950).
// Replaces torch.nn.GroupNorm / F.silu / LayerNorm inside diffusers' ResnetBlock2D, Transformer2DModel,
// AutoencoderKL decoder (reference call sites generate_data.py:112, :701) and their autograd backward (:721).
// HBM-bound: 16-byte vector loads, fp32 statistics, deterministic two-stage reductions (no float atomics
// anywhere, so results are bitwise reproducible run to run).
//
// GroupNorm is three passes, each a kernel of its own: pass 1 gn_partial_kernel (per split of rows), pass 2 gn_finalize_stats_kernel /
// gn_finalize_bwd_kernel (or, from the convolutions' channel partials, gn_finalize_chan_kernel for passes 1 + 2), pass 3 gn_apply_kernel.
// Passes 1 and 3 share the column map (GnCols) and the backward element (norm_bwd_elem); pass 1 walks its rows with gn_walk_rows, pass 3
// keeps the same walk written out (its comment says why).
#include "common.h"
#include "kernels.h"

namespace {

constexpr int GN_THREADS = 256;
constexpr int GN_MAX_SPLIT = 256;
#define NORM_FUNCTOR_INLINE __attribute__((always_inline))   // on a lambda: the functors of the walks below must inline away (their captures are registers)

// rows per partial block: ~32K elements per block so that mid-size tensors still spread over hundreds of blocks
__host__ __device__ inline int gn_split(int HW, int C) {
  int rows = 32768 / C;
  if (rows < 4) rows = 4;
  int s = (HW + rows - 1) / rows;
  if (s < 1) s = 1;
  if (s > GN_MAX_SPLIT) s = GN_MAX_SPLIT;
  return s;
}

// Column ownership of the streaming passes: a thread owns one 8-channel vector column (my_vc0, and my_vc0 + VCt, ... when C / 8 > 256)
// and every R-th row from my_r; the 256 % VCt threads with my_r >= R are idle.
struct GnCols {
  int VC, VCt, R, my_r, my_vc0;
  __host__ __device__ GnCols(int C, int tid) : VC(C >> 3), VCt(VC < GN_THREADS ? VC : GN_THREADS), R(GN_THREADS / VCt), my_r(tid / VCt), my_vc0(tid % VCt) {}
};

// The row walk of pass 1 (and, written out, of pass 3): rows first, first + step, ... below end, four in flight per thread (memory-level parallelism):
// load(raw, row, live) fills the N 16-byte vectors of each of the four slots (live: row < end), then body(raw, row) runs for the live
// ones in row order, so accumulation order stays fixed.
template <int N, class Load, class Body>
__device__ __forceinline__ void gn_walk_rows(int first, int end, int step, Load load, Body body) {
  for (int row0 = first; row0 < end; row0 += 4 * step) {
    uint4 raw[4][N];
#pragma unroll
    for (int u = 0; u < 4; ++u) load(raw[u], row0 + u * step, row0 + u * step < end);
    __builtin_amdgcn_sched_barrier(0);   // load all, then compute: no unpack of the first row moves in between the loads (it waits for its load alone)
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (row0 + u * step < end) body(raw[u], row0 + u * step);
  }
}

// The backward element of GroupNorm(+SiLU) and LayerNorm: xh = xhat, da = dy act'(xhat gamma + beta), d = da gamma.  Pass 1 sums d and
// d * xh, pass 3 (and the LayerNorm backward) recomputes both and subtracts the means of those sums: xh, da and d come from this one
// expression, so they cannot drift.  What pass 1 adds to its first sum is not d as rounded here, though: it is da * gamma inside one fused
// multiply-add (the recorded bits hold that contraction, see there), so `da` is given out beside d.
struct BwdElem { float xh, da, d; };
__device__ __forceinline__ BwdElem norm_bwd_elem(float x, float dy, float mean, float rstd, float ga, float be, bool silu) {
  BwdElem q;
  q.xh = (x - mean) * rstd;
  q.da = dy;
  if (silu) q.da *= dsilu_f(q.xh * ga + be);
  q.d = q.da * ga;
  return q;
}

// Pass 1 (fwd): per (b, split, group) partial (count, mean, M2).
// Pass 1 (bwd): per (b, split, group) partial (s1 = sum dxhat, s2 = sum dxhat*xhat).
template <bool BWD>
__global__ __launch_bounds__(GN_THREADS) void gn_partial_kernel(GroupNormParams p) {
  // sh[r][2][C]: per staging-row partial sums, combined in a fixed order (no atomics: bitwise reproducible)
  extern __shared__ float sh[];
  const int C = p.C, G = p.G, cpg = C / G;
  const int b = blockIdx.y, s = blockIdx.x, S = gridDim.x;
  const int rows_per = (p.HW + S - 1) / S;
  const int row_begin = s * rows_per, row_end = min(p.HW, row_begin + rows_per);
  const GnCols col(C, threadIdx.x);
  if (col.my_r < col.R) {
    for (int vc = col.my_vc0; vc < col.VC; vc += col.VCt) {
      float a0[8], a1[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { a0[e] = 0.f; a1[e] = 0.f; }
      float ga[8], be[8], mean[8], rstd[8];
      if (BWD) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int c = vc * 8 + e, g = c / cpg;
          ga[e] = p.gamma[c]; be[e] = p.beta[c];
          mean[e] = p.stats[((size_t)b * G + g) * 2]; rstd[e] = p.stats[((size_t)b * G + g) * 2 + 1];
        }
      }
      gn_walk_rows<BWD ? 2 : 1>(
          row_begin + col.my_r, row_end, col.R,
          [&](uint4* raw, int row, bool live) NORM_FUNCTOR_INLINE {
            const size_t pix = (size_t)b * p.HW + (live ? row : row_begin);   // a dead slot loads the split's first row again
            raw[0] = *(const uint4*)(p.x + pix * p.x_ld + vc * 8);
            if constexpr (BWD) raw[1] = *(const uint4*)(p.dy + pix * p.dy_ld + vc * 8);
          },
          [&](const uint4* raw, int) NORM_FUNCTOR_INLINE {
            float xv[8];
            unpack8(raw[0], xv);
            if constexpr (!BWD) {
#pragma unroll
              for (int e = 0; e < 8; ++e) { a0[e] += xv[e]; a1[e] += xv[e] * xv[e]; }
            } else {
              float dv[8];
              unpack8(raw[1], dv);
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                // the two sums as the fused operations they have in the recorded bits, a0 += da * gamma and a1 += d * xh in one rounding
                // each: written `+=`, whether they fuse is the vectoriser's choice (it pairs the adds when the body comes from a functor)
                const BwdElem q = norm_bwd_elem(xv[e], dv[e], mean[e], rstd[e], ga[e], be[e], p.silu);
                a0[e] = fmaf(q.da, ga[e], a0[e]); a1[e] = fmaf(q.d, q.xh, a1[e]);
              }
            }
          });
      float* dst = sh + (size_t)col.my_r * 2 * C;
#pragma unroll
      for (int e = 0; e < 8; ++e) { dst[vc * 8 + e] = a0[e]; dst[C + vc * 8 + e] = a1[e]; }
    }
  }
  __syncthreads();
  for (int g = threadIdx.x; g < G; g += GN_THREADS) {
    float t0 = 0.f, t1 = 0.f;
    for (int r = 0; r < col.R; ++r) {
      const float* src = sh + (size_t)r * 2 * C;
      for (int c = g * cpg; c < (g + 1) * cpg; ++c) { t0 += src[c]; t1 += src[C + c]; }
    }
    float* out = p.scratch + (((size_t)b * S + s) * G + g) * 3;
    if (!BWD) {
      const float n = (float)(row_end - row_begin) * cpg;
      const float m = n > 0 ? t0 / n : 0.f;
      out[0] = n; out[1] = m; out[2] = fmaxf(t1 - t0 * m, 0.f);  // M2 = sumsq - n*mean^2
    } else {
      out[0] = t0; out[1] = t1; out[2] = 0.f;
    }
  }
}

// Pass 2: one wave per (b, g) merges the S partials of pass 1 in a fixed tree order.  Which (b, g) a wave has, where its partials lie
// and where its pair of results goes:
struct GnWave {
  int lane, b, g, G;
  bool live;
  __device__ explicit GnWave(const GroupNormParams& p) : lane(threadIdx.x & 63), G(p.G) {
    const int bg = blockIdx.x * (GN_THREADS / 64) + (threadIdx.x >> 6);
    live = bg < p.B * p.G; b = bg / p.G; g = bg % p.G;
  }
  __device__ const float* partial(const float* scratch, int S, int s) const { return scratch + (((size_t)b * S + s) * G + g) * 3; }
  __device__ size_t pair() const { return ((size_t)b * G + g) * 2; }
};

// Pass 2 (fwd): Chan et al. parallel merge of (n, mean, M2) -> stats[b][g] = (mean, rstd).  The two merges below are not one function:
// the lane's own sequential merge adds M2 + (M2b + t), the butterfly (lo_M + hi_M) + t with both partners in the same operand order;
// they associate differently, and the recorded bits (tests/golden/norm_bits.npz) hold each as it is.
__global__ __launch_bounds__(GN_THREADS) void gn_finalize_stats_kernel(GroupNormParams p, int S) {
  const GnWave w(p);
  if (!w.live) return;
  const int lane = w.lane;
  float n = 0.f, mean = 0.f, M2 = 0.f;
  for (int s = lane; s < S; s += 64) {
    const float* in = w.partial(p.scratch, S, s);
    const float nb = in[0], mb = in[1], M2b = in[2];
    if (nb > 0.f) {
      const float nn = n + nb, d = mb - mean;
      mean += d * (nb / nn);
      M2 += M2b + d * d * (n * nb / nn);
      n = nn;
    }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float nb = __shfl_xor(n, o, 64), mb = __shfl_xor(mean, o, 64), M2b = __shfl_xor(M2, o, 64);
    // symmetric merge (both partners compute the same result, in the same operand order)
    const float nn = n + nb;
    if (nn > 0.f) {
      const float lo_n = (lane & o) ? nb : n, hi_n = (lane & o) ? n : nb;
      const float lo_m = (lane & o) ? mb : mean, hi_m = (lane & o) ? mean : mb;
      const float lo_M = (lane & o) ? M2b : M2, hi_M = (lane & o) ? M2 : M2b;
      const float d = hi_m - lo_m;
      mean = lo_m + d * (hi_n / nn);
      M2 = lo_M + hi_M + d * d * (lo_n * hi_n / nn);
      n = nn;
    }
  }
  if (lane == 0) {
    p.stats[w.pair()] = mean;
    p.stats[w.pair() + 1] = rsqrtf(M2 / n + p.eps);
  }
}

// Pass 2 (bwd): sums -> fin[b][g] = (s1/n, s2/n)
__global__ __launch_bounds__(GN_THREADS) void gn_finalize_bwd_kernel(GroupNormParams p, int S, float* fin) {
  const GnWave w(p);
  if (!w.live) return;
  float s1 = 0.f, s2 = 0.f;
  for (int s = w.lane; s < S; s += 64) {
    const float* in = w.partial(p.scratch, S, s);
    s1 += in[0]; s2 += in[1];
  }
  s1 = wave_sum(s1); s2 = wave_sum(s2);
  if (w.lane == 0) {
    const float n = (float)p.HW * (p.C / p.G);
    fin[w.pair()] = s1 / n;
    fin[w.pair() + 1] = s2 / n;
  }
}

// Pass 1+2 when the producing convolutions emitted per-(64-row block, channel) partials (mean, M2 over 64 rows; CF_STATS of the
// implicit-GEMM epilogue): one 256-thread workgroup per (b, g) merges the (HW / 64) x (C / G) partials of its group, no pass over the
// tensor.  All partials have the same count, so the merge is mean = avg(mean_p), M2 = sum(M2_p) + 64 * sum((mean_p - mean)^2), with
// every thread's partials held in registers between the two reductions; fixed-order wave + LDS sums (bitwise reproducible).
// gn_block_sum pairs the four wave sums; block_sum in elementwise.hip adds red[0..n) left to right.  The two give different bits, so
// they stay two functions.
__device__ __forceinline__ float gn_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(GN_THREADS) void gn_finalize_chan_kernel(GroupNormParams p) {
  __shared__ float red[4];
  const int bg = blockIdx.x;
  const int b = bg / p.G, g = bg % p.G;
  const int cpg = p.C / p.G, nb = p.HW >> 6, P = nb * cpg;
  constexpr int MAXP = 12;                       // partials per thread kept in registers (P <= 3072); beyond that they are re-read
  float pm[MAXP], pM[MAXP];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAXP; ++i) {
    const int e = threadIdx.x + i * GN_THREADS;
    pm[i] = 0.f; pM[i] = 0.f;
    if (e < P) {
      const int rb = e / cpg, c = g * cpg + (e - rb * cpg);
      const float2 in = *(const float2*)(p.chan_part + (((size_t)b * nb + rb) * p.part_ld + c) * 2);
      pm[i] = in.x; pM[i] = in.y; s += in.x;
    }
  }
  for (int e = threadIdx.x + MAXP * GN_THREADS; e < P; e += GN_THREADS) {
    const int rb = e / cpg, c = g * cpg + (e - rb * cpg);
    s += p.chan_part[(((size_t)b * nb + rb) * p.part_ld + c) * 2];
  }
  const float mean = gn_block_sum(s, red) / (float)P;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < MAXP; ++i) {
    const int e = threadIdx.x + i * GN_THREADS;
    if (e < P) { const float d = pm[i] - mean; q += pM[i] + 64.f * d * d; }
  }
  for (int e = threadIdx.x + MAXP * GN_THREADS; e < P; e += GN_THREADS) {
    const int rb = e / cpg, c = g * cpg + (e - rb * cpg);
    const float2 in = *(const float2*)(p.chan_part + (((size_t)b * nb + rb) * p.part_ld + c) * 2);
    const float d = in.x - mean;
    q += in.y + 64.f * d * d;
  }
  const float M2 = gn_block_sum(q, red);
  if (threadIdx.x == 0) {
    p.stats[((size_t)b * p.G + g) * 2] = mean;
    p.stats[((size_t)b * p.G + g) * 2 + 1] = rsqrtf(fmaxf(M2, 0.f) / (64.f * (float)P) + p.eps);
  }
}

// Pass 3: build the per-channel coefficients in LDS, stream the tensor (4 vectors in flight per thread).  The LDS rows, C floats each
// (gn_launch sizes the LDS from the same counts):
enum { GN_SCALE, GN_SHIFT, GN_FWD_ROWS };                                  // fwd: y = x * scale + shift
enum { GN_GAMMA, GN_MEAN, GN_RSTD, GN_S1, GN_S2, GN_BETA, GN_BWD_ROWS };   // bwd: s1 = sum d / n, s2 = sum d xhat / n
template <bool BWD>
__global__ __launch_bounds__(GN_THREADS) void gn_apply_kernel(GroupNormParams p, const float* fin) {
  extern __shared__ float sh[];
  const int C = p.C, G = p.G, cpg = C / G;
  const int b = blockIdx.y;
  for (int c = threadIdx.x; c < C; c += GN_THREADS) {
    const int g = c / cpg;
    const float mean = p.stats[((size_t)b * G + g) * 2], rstd = p.stats[((size_t)b * G + g) * 2 + 1];
    if (!BWD) {
      const float a = rstd * p.gamma[c];
      sh[GN_SCALE * C + c] = a; sh[GN_SHIFT * C + c] = p.beta[c] - mean * a;
    } else {
      sh[GN_GAMMA * C + c] = p.gamma[c]; sh[GN_MEAN * C + c] = mean; sh[GN_RSTD * C + c] = rstd; sh[GN_BETA * C + c] = p.beta[c];
      sh[GN_S1 * C + c] = fin[((size_t)b * G + g) * 2]; sh[GN_S2 * C + c] = fin[((size_t)b * G + g) * 2 + 1];
    }
  }
  __syncthreads();
  // a thread owns one 8-channel vector column and walks rows: its 16 (or 48) coefficients live in registers for the whole sweep, no
  // per-vector index division, no LDS traffic in the streaming loop (the kernel was VALU/LDS-bound at ~2.8 TB/s before).
  // The walk is gn_walk_rows written out, and the coefficients are six arrays, on purpose: through the functors of gn_walk_rows, or with
  // the coefficients as one co[rows][8], the compiler waits for all the LDS reads below in front of the first global loads (the code
  // as written leaves the last four in flight across them), and the backward launches with an uncapped grid measured 2 to 2.7 % slower
  // 
  const GnCols col(C, threadIdx.x);
  if (col.my_r >= col.R) return;
  const int rstep = gridDim.x * col.R;
  for (int vc = col.my_vc0; vc < col.VC; vc += col.VCt) {
    float ca[8], cb[8], cc[8], cd[8], ce[8], cf[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = vc * 8 + e;
      ca[e] = sh[GN_SCALE * C + c]; cb[e] = sh[GN_SHIFT * C + c];      // bwd: GN_GAMMA, GN_MEAN
      if (BWD) { cc[e] = sh[GN_RSTD * C + c]; cd[e] = sh[GN_S1 * C + c]; ce[e] = sh[GN_S2 * C + c]; cf[e] = sh[GN_BETA * C + c]; }
    }
    for (int row0 = blockIdx.x * col.R + col.my_r; row0 < p.HW; row0 += 4 * rstep) {
      uint4 xr[4], dr[4], orr[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int row = row0 + u * rstep;
        if (row < p.HW) {
          const size_t pix = (size_t)b * p.HW + row;
          xr[u] = *(const uint4*)(p.x + pix * p.x_ld + vc * 8);
          if (BWD) {
            dr[u] = *(const uint4*)(p.dy + pix * p.dy_ld + vc * 8);
            if (p.accumulate) orr[u] = *(const uint4*)(p.dx + pix * p.dx_ld + vc * 8);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int row = row0 + u * rstep;
        if (row >= p.HW) continue;
        const size_t pix = (size_t)b * p.HW + row;
        float xv[8], ov[8];
        unpack8(xr[u], xv);
        if (!BWD) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float y = xv[e] * ca[e] + cb[e];
            ov[e] = p.silu ? silu_f(y) : y;
          }
          *(uint4*)(p.y + pix * p.y_ld + vc * 8) = pack8(ov);
        } else {
          float dv[8];
          unpack8(dr[u], dv);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const BwdElem q = norm_bwd_elem(xv[e], dv[e], cb[e], cc[e], ca[e], cf[e], p.silu);
            ov[e] = cc[e] * (q.d - cd[e] - q.xh * ce[e]);
          }
          if (p.accumulate) {
            float old[8];
            unpack8(orr[u], old);
#pragma unroll
            for (int e = 0; e < 8; ++e) ov[e] += old[e];
          }
          *(uint4*)(p.dx + pix * p.dx_ld + vc * 8) = pack8(ov);
        }
      }
    }
  }
}

// ---------------- LayerNorm: one wave per row (forward: per LN_RPW rows), a lane holds up to VI <= 4 vectors of it: 4 x 64 x 8 = 2048 channels
// f(i, vc) for the lane's i-th vector, column vc = lane + 64 i, where the row has one
template <int VI, class F>
__device__ __forceinline__ void ln_each_vec(int lane, int VC, F f) {
#pragma unroll
  for (int i = 0; i < VI; ++i) {
    const int vc = lane + 64 * i;
    if (vc < VC) f(i, vc);
  }
}
// eight consecutive floats of gamma / beta (32-byte aligned: C % 8 == 0)
__device__ __forceinline__ void load8f(const float* src, float* v) {
  const float4 lo = *(const float4*)src, hi = *(const float4*)(src + 4);
  v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
}

// Forward: a wave takes LN_RPW consecutive rows, all their loads in flight at once (a 320-channel row is only 640 bytes: one row per
// wave left the kernel latency-bound), gamma / beta in registers
constexpr int LN_RPW = 4;
template <int VI>
__global__ __launch_bounds__(256) void ln_rows_kernel(LayerNormParams p) {
  const int lane = threadIdx.x & 63;
  const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * LN_RPW;
  if (row0 >= p.M) return;
  const int VC = p.C >> 3;
  const bool stats_only = p.y == nullptr;     // the LayerNorm is folded into the GEMM that follows (CF_LNFOLD): statistics only
  float ga[VI][8], be[VI][8];
  if (!stats_only) ln_each_vec<VI>(lane, VC, [&](int i, int vc) NORM_FUNCTOR_INLINE { load8f(p.gamma + vc * 8, ga[i]); load8f(p.beta + vc * 8, be[i]); });
  uint4 raw[LN_RPW][VI];
#pragma unroll
  for (int r = 0; r < LN_RPW; ++r) {
#pragma unroll
    for (int i = 0; i < VI; ++i) raw[r][i] = make_uint4(0, 0, 0, 0);
    if (row0 + r < p.M) ln_each_vec<VI>(lane, VC, [&](int i, int vc) NORM_FUNCTOR_INLINE { raw[r][i] = *(const uint4*)(p.x + (size_t)(row0 + r) * p.x_ld + vc * 8); });
  }
#pragma unroll
  for (int r = 0; r < LN_RPW; ++r) {
    const int row = row0 + r;
    if (row >= p.M) break;                    // wave-uniform
    float xv[VI][8];
#pragma unroll
    for (int i = 0; i < VI; ++i) unpack8(raw[r][i], xv[i]);
    float s = 0.f;
    ln_each_vec<VI>(lane, VC, [&](int i, int) NORM_FUNCTOR_INLINE {
#pragma unroll
      for (int e = 0; e < 8; ++e) s += xv[i][e];
    });
    const float mean = wave_sum(s) / p.C;
    float v = 0.f;
    ln_each_vec<VI>(lane, VC, [&](int i, int) NORM_FUNCTOR_INLINE {
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = xv[i][e] - mean; v += d * d; }
    });
    const float rstd = rsqrtf(wave_sum(v) / p.C + p.eps);
    if (lane == 0 && p.stats) { p.stats[(size_t)row * 2] = mean; p.stats[(size_t)row * 2 + 1] = rstd; }
    if (stats_only) continue;
    ln_each_vec<VI>(lane, VC, [&](int i, int vc) NORM_FUNCTOR_INLINE {
      float ov[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) ov[e] = (xv[i][e] - mean) * rstd * ga[i][e] + be[i][e];
      *(uint4*)(p.y + (size_t)row * p.y_ld + vc * 8) = pack8(ov);
    });
  }
}

// Backward: one row per wave, from the forward's (mean, rstd); the element is norm_bwd_elem without activation.  Its three per-lane
// loops stay plain loops, not ln_each_vec: from a functor the vectoriser pairs the adds of the sums, some `s1 += d` fuse with the product
// that made d and dx leaves the recorded bits (tests/golden/norm_bits.npz); with the helper on the other two loops alone the second
// vector's dy and gamma loads are no longer issued together and the kernel was 6 % slower
__global__ __launch_bounds__(256) void ln_bwd_kernel(LayerNormParams p) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.M) return;
  const int VC = p.C >> 3;
  float xv[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int vc = lane + 64 * i;
    if (vc < VC) unpack8(*(const uint4*)(p.x + (size_t)row * p.x_ld + vc * 8), xv[i]);
  }
  const float mean = p.stats[(size_t)row * 2], rstd = p.stats[(size_t)row * 2 + 1];
  float dv[4][8];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int vc = lane + 64 * i;
    if (vc < VC) {
      unpack8(*(const uint4*)(p.dy + (size_t)row * p.dy_ld + vc * 8), dv[i]);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const BwdElem q = norm_bwd_elem(xv[i][e], dv[i][e], mean, rstd, p.gamma[vc * 8 + e], 0.f, false);
        dv[i][e] = q.d; xv[i][e] = q.xh;
        s1 += q.d; s2 += q.d * q.xh;
      }
    }
  }
  s1 = wave_sum(s1) / p.C; s2 = wave_sum(s2) / p.C;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int vc = lane + 64 * i;
    if (vc < VC) {
      float ov[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) ov[e] = rstd * (dv[i][e] - s1 - xv[i][e] * s2);
      bf16_t* dst = p.dx + (size_t)row * p.dx_ld + vc * 8;
      if (p.accumulate) {
        float old[8];
        unpack8(*(const uint4*)dst, old);
#pragma unroll
        for (int e = 0; e < 8; ++e) ov[e] += old[e];
      }
      *(uint4*)dst = pack8(ov);
    }
  }
}

}  // namespace

size_t groupnorm_scratch_bytes(int B, int G) { return ((size_t)B * GN_MAX_SPLIT * G * 3 + (size_t)B * G * 2) * sizeof(float); }

static size_t gn_partial_lds(int C) { return (size_t)GnCols(C, 0).R * 2 * C * sizeof(float); }
// Refused in front of any launch (and of any division by G): empty or negative extents, more images than a grid's y extent holds, a
// channel count that is no whole number of 8-channel vectors or of groups, a row stride that would misalign the 16-byte accesses.
static hipError_t gn_check(const GroupNormParams& p) {
  if (p.G <= 0 || p.C <= 0 || p.HW <= 0 || p.B <= 0 || p.B > 65535) return hipErrorInvalidValue;
  if (p.C % 8 || p.C % p.G || (p.x_ld & 7)) return hipErrorInvalidValue;
  return hipSuccess;
}
static int gn_apply_blocks(const GroupNormParams& p) {
  int blocks = (p.HW * (p.C / 8) + GN_THREADS * 8 - 1) / (GN_THREADS * 8);
  if (blocks < 1) blocks = 1;
  constexpr int total = 4096;   // blocks per launch over all images (2048 -> 4096: norm family 265 -> 260 ms per 32-image batch)
  const int cap = total / (p.B > 0 ? p.B : 1) + 1;
  if (blocks > cap) blocks = cap;
  return blocks;
}

template <bool BWD>
static hipError_t gn_launch(const GroupNormParams& p, hipStream_t stream) {
  const int S = gn_split(p.HW, p.C);
  float* fin = p.scratch + (size_t)p.B * GN_MAX_SPLIT * p.G * 3;   // [B][G][2] finalize output of the backward sums
  const dim3 waves((p.B * p.G + 3) / 4);                           // pass 2: one wave per (b, g)
  if (!BWD && p.chan_part) {
    hipLaunchKernelGGL(gn_finalize_chan_kernel, dim3(p.B * p.G), dim3(GN_THREADS), 0, stream, p);
  } else {
    hipLaunchKernelGGL((gn_partial_kernel<BWD>), dim3(S, p.B), dim3(GN_THREADS), gn_partial_lds(p.C), stream, p);
    if (BWD) {
      hipLaunchKernelGGL(gn_finalize_bwd_kernel, waves, dim3(GN_THREADS), 0, stream, p, S, fin);
    } else {
      hipLaunchKernelGGL(gn_finalize_stats_kernel, waves, dim3(GN_THREADS), 0, stream, p, S);
    }
  }
  hipLaunchKernelGGL((gn_apply_kernel<BWD>), dim3(gn_apply_blocks(p), p.B), dim3(GN_THREADS), (BWD ? GN_BWD_ROWS : GN_FWD_ROWS) * p.C * sizeof(float),
                     stream, p, (const float*)fin);
  return hipGetLastError();
}

hipError_t launch_groupnorm_fwd(const GroupNormParams& p, hipStream_t stream) {
  if (gn_check(p) != hipSuccess || (p.y_ld & 7)) return hipErrorInvalidValue;
  if (p.chan_part && (p.HW & 63)) return hipErrorInvalidValue;     // the partials are per 64-row block
  return gn_launch<false>(p, stream);
}

hipError_t launch_groupnorm_bwd(const GroupNormParams& p, hipStream_t stream) {
  if (gn_check(p) != hipSuccess || (p.dy_ld & 7) || (p.dx_ld & 7)) return hipErrorInvalidValue;
  return gn_launch<true>(p, stream);
}

// (mean, rstd) of every row from the (sum, sum^2) partials the producing GEMM emitted per column span (CF_ROWSTATS): M x spans x 8 bytes
// read instead of the M x C x 2 of a pass over the tensor.  fp32 sums of the fp32 values in front of their bf16 rounding.
__global__ __launch_bounds__(256) void ln_rowpart_finalize_kernel(LayerNormParams p) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= p.M) return;
  const float2* pp = (const float2*)p.rowpart + (size_t)row * p.rowpart_ld;
  float a = 0.f, q = 0.f;
  for (int s = 0; s < p.spans; ++s) { const float2 v = pp[s]; a += v.x; q += v.y; }
  const float mean = a / p.C;
  const float var = fmaxf(q / p.C - mean * mean, 0.f);
  *(float2*)(p.stats + (size_t)row * 2) = make_float2(mean, rsqrtf(var + p.eps));
}

// Refused by both LayerNorm launchers: empty extents, a row that is no whole number of 8-channel vectors or wider than the 4 vectors a
// lane holds, an x stride that would misalign the 16-byte accesses.
static hipError_t ln_check(const LayerNormParams& p) {
  if (p.M <= 0 || p.C <= 0 || p.C % 8 || p.C > 2048 || (p.x_ld & 7)) return hipErrorInvalidValue;
  return hipSuccess;
}

hipError_t launch_layernorm_fwd(const LayerNormParams& p, hipStream_t stream) {
  if (ln_check(p) != hipSuccess || (p.y && (p.y_ld & 7)) || (!p.y && !p.stats)) return hipErrorInvalidValue;
  if (!p.y && p.rowpart) {
    if (p.spans < 1 || p.rowpart_ld < p.spans) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ln_rowpart_finalize_kernel, dim3((p.M + 255) / 256), dim3(256), 0, stream, p);
    return hipGetLastError();
  }
  const dim3 blocks((p.M + 4 * LN_RPW - 1) / (4 * LN_RPW));
  switch ((p.C / 8 + 63) / 64) {              // vectors per lane: 1..4 (ln_check: C <= 2048)
    case 1: hipLaunchKernelGGL((ln_rows_kernel<1>), blocks, dim3(256), 0, stream, p); break;
    case 2: hipLaunchKernelGGL((ln_rows_kernel<2>), blocks, dim3(256), 0, stream, p); break;
    case 3: hipLaunchKernelGGL((ln_rows_kernel<3>), blocks, dim3(256), 0, stream, p); break;
    default: hipLaunchKernelGGL((ln_rows_kernel<4>), blocks, dim3(256), 0, stream, p); break;
  }
  return hipGetLastError();
}

hipError_t launch_layernorm_bwd(const LayerNormParams& p, hipStream_t stream) {
  if (ln_check(p) != hipSuccess || (p.dy_ld & 7) || (p.dx_ld & 7) || !p.stats) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ln_bwd_kernel, dim3((p.M + 3) / 4), dim3(256), 0, stream, p);
  return hipGetLastError();
}

#undef NORM_FUNCTOR_INLINE
