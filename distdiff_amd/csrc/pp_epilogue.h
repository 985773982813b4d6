// Epilogue shared by the ping-pong kernels: conv_halo_kernel / conv_halo_persist_kernel (conv_halo.hip) and gemm_pps_kernel (gemm_pps.hip).
#pragma once
#include "common.h"
#include "kernels.h"

// Shared epilogue of the ping-pong kernels: a lane owns, per 16-row tile a, 8 consecutive channels of a tile pair (16-byte loads /
// stores) and 4 of an odd last tile.  bias / residual / ReLU / CF_STATS (GroupNorm partials per 64-row block) as in conv_gemm2.hip, plus
// CF_LNFOLD (out = rstd[m] * (acc - mean[m] * c1[n]) + b'[n]: the LayerNorm in front of this linear is folded into its weights) and
// CF_ROWSTATS ((sum, sum^2) of every output row over this wave's TN * 16 columns, for the LayerNorm that consumes the tensor).
// stats_s: the (mean, rstd) rows of the tile in LDS (persistent GEMM: they arrive with the bias through the LDS-DMA ring), or null (global loads).
// LA: 16-row tiles whose residual rows / statistics are requested together (2: one exposed memory latency per 32 rows; 4: per 64 rows --
// 16 more registers, which only the TN = 4 forms have: with TN = 5 it spilled)
// sblk_of(r): CF_STATS block slot ([M / 64] of p.stats) of the 64 tile rows r .. r + 63 (r a multiple of 64)
template <int TN, int LA = 2, class MOf, class SOf>
__device__ __forceinline__ void pp_epilogue(const ConvGemmParams& p, f32x4 (&acc)[8][TN], MOf m_of, SOf sblk_of, int wr, int wc, int n0,
                                            const float* bias_s, const float* c1_s, int span, int fr, int fq, const float* stats_s = nullptr) {
  constexpr int TNP = TN & ~1;
  const int fl = p.flags;
  const int wb = n0 + wc * (TN * 16);
  const float* bw = bias_s + wc * (TN * 16);
  const float* cw = c1_s + wc * (TN * 16);
#pragma unroll
  for (int blk = 0; blk < 2; ++blk) {                   // 64-row blocks (the granule of the GroupNorm partials)
    float s1[TN][4], s2[TN][4];
#pragma unroll
    for (int jn = 0; jn < TN; ++jn)
#pragma unroll
      for (int r = 0; r < 4; ++r) { s1[jn][r] = 0.f; s2[jn][r] = 0.f; }
#pragma unroll
    for (int hb = 0; hb < 4 / LA; ++hb) {
    // the residual rows / LayerNorm statistics of LA 16-row tiles are requested before their first use: one exposed memory latency per
    // 32 (64) rows instead of one per tile pair (the accumulators and the GroupNorm sums leave ~50 registers free here)
    uint4 rvp[LA][TN / 2];
    uint2 rvo[LA];
    float2 lst[LA];
    int mrow[LA];
#pragma unroll
    for (int a4 = 0; a4 < LA; ++a4) {
      mrow[a4] = m_of(wr * 128 + (blk * 4 + hb * LA + a4) * 16 + fr);
      const bf16_t* rp = (const bf16_t*)p.res + (size_t)mrow[a4] * p.res_ld + wb;
      if (fl & CF_RES) {
#pragma unroll
        for (int t = 0; t < TN / 2; ++t) rvp[a4][t] = *(const uint4*)(rp + t * 32 + fq * 8);
        if constexpr (TN & 1) rvo[a4] = *(const uint2*)(rp + (TN - 1) * 16 + fq * 4);
      } else {
#pragma unroll
        for (int t = 0; t < TN / 2; ++t) rvp[a4][t] = make_uint4(0, 0, 0, 0);
        rvo[a4] = make_uint2(0, 0);
      }
      lst[a4] = !(fl & CF_LNFOLD) ? make_float2(0.f, 1.f)
                : stats_s ? *(const float2*)(stats_s + (wr * 128 + (blk * 4 + hb * LA + a4) * 16 + fr) * 2) : *(const float2*)(p.ln_stats + (size_t)mrow[a4] * 2);
    }
#pragma unroll
    for (int a4 = 0; a4 < LA; ++a4) {
      const int a = blk * 4 + hb * LA + a4;
      const int m = mrow[a4];
      bf16_t* yp = (bf16_t*)p.y + (size_t)m * p.y_ld;
      const float rs = lst[a4].y * p.alpha, nm = -rs * lst[a4].x;      // CF_LNFOLD: alpha * rstd and -alpha * rstd * mean of this lane's row (alpha, 0 otherwise)
      float r1 = 0.f, r2 = 0.f;                          // CF_ROWSTATS
      auto four = [&](const f32x4& v, int col, unsigned q0, unsigned q1, float* t1, float* t2) {
        float4 b = *(const float4*)(bw + col);
        if (fl & CF_LNFOLD) {
          const float4 c = *(const float4*)(cw + col);
          b.x = __builtin_fmaf(nm, c.x, b.x); b.y = __builtin_fmaf(nm, c.y, b.y); b.z = __builtin_fmaf(nm, c.z, b.z); b.w = __builtin_fmaf(nm, c.w, b.w);
        }
        float v0 = __builtin_fmaf(v[0], rs, b.x), v1 = __builtin_fmaf(v[1], rs, b.y), v2 = __builtin_fmaf(v[2], rs, b.z), v3 = __builtin_fmaf(v[3], rs, b.w);
        if (fl & CF_RES) {
          add_res4(q0, q1, v0, v1, v2, v3);
        }
        if (fl & CF_RELU) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f); }
        if (fl & CF_STATS) {
          DD_STORED4(v0, v1, v2, v3, u0, u1, u2, u3);
          t1[0] += u0; t1[1] += u1; t1[2] += u2; t1[3] += u3;
          t2[0] = __builtin_fmaf(u0, u0, t2[0]); t2[1] = __builtin_fmaf(u1, u1, t2[1]);
          t2[2] = __builtin_fmaf(u2, u2, t2[2]); t2[3] = __builtin_fmaf(u3, u3, t2[3]);
        }
        if (fl & CF_ROWSTATS) {
          r1 += (v0 + v1) + (v2 + v3);
          r2 = __builtin_fmaf(v0, v0, __builtin_fmaf(v1, v1, __builtin_fmaf(v2, v2, __builtin_fmaf(v3, v3, r2))));
        }
        return make_uint2(pack2bf(v0, v1), pack2bf(v2, v3));
      };
#pragma unroll
      for (int t = 0; t < TN / 2; ++t) {
        const int col = t * 32 + fq * 8;                // column of the pair's first value inside the wave's span
        const uint4 rv = rvp[a4][t];
        const uint2 lo = four(acc[a][2 * t], col, rv.x, rv.y, s1[2 * t], s2[2 * t]);
        const uint2 hi = four(acc[a][2 * t + 1], col + 4, rv.z, rv.w, s1[2 * t + 1], s2[2 * t + 1]);
        *(uint4*)(yp + wb + col) = make_uint4(lo.x, lo.y, hi.x, hi.y);
      }
      if constexpr (TN & 1) {
        const int col = (TN - 1) * 16 + fq * 4;
        *(uint2*)(yp + wb + col) = four(acc[a][TN - 1], col, rvo[a4].x, rvo[a4].y, s1[TN - 1], s2[TN - 1]);
      }
      if (fl & CF_ROWSTATS) {
        // the row's TN * 16 columns of this wave sit in lanes fr, fr + 16, fr + 32, fr + 48
        r1 += __shfl_xor(r1, 16, 64); r2 += __shfl_xor(r2, 16, 64);
        r1 += __shfl_xor(r1, 32, 64); r2 += __shfl_xor(r2, 32, 64);
        if (fq == 0) *(float2*)(p.rowpart + ((size_t)m * p.rowpart_ld + span) * 2) = make_float2(r1, r2);
      }
    }
    }
    if (fl & CF_STATS) {
      // per-(64-row block, channel) (mean, M2) of the stored values for the GroupNorm that consumes this tensor (conv_gemm2.hip emit_stats)
      float* dst0 = p.stats + ((size_t)sblk_of(wr * 128 + blk * 64) * p.stats_ld) * 2;
#pragma unroll
      for (int jn = 0; jn < TN; ++jn) {
        float o[8];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float sa = row16_sum(s1[jn][r]), sq = row16_sum(s2[jn][r]);
          const float mean = sa * (1.f / 64.f);
          o[2 * r] = mean; o[2 * r + 1] = fmaxf(sq - sa * mean, 0.f);
        }
        const int col = jn < TNP ? (jn >> 1) * 32 + fq * 8 + (jn & 1) * 4 : jn * 16 + fq * 4;
        if (fr == 0) {
          float* dst = dst0 + (size_t)(wb + col) * 2;                  // p.stats is already offset to this op's first channel
          *(float4*)dst = make_float4(o[0], o[1], o[2], o[3]);
          *(float4*)(dst + 4) = make_float4(o[4], o[5], o[6], o[7]);
        }
      }
    }
  }
}
