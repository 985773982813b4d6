// K2/K8 (pointwise layers) -- persistent ping-pong GEMM for 1x1 convolutions / linear layers, bf16 MFMA, gfx950: the phase-alternating
// K loop of conv_halo.hip (its header says why) with both operands streamed: the K-step is pp_kstep of pp_kloop.h, which the halo kernels
// run too, and the epilogue the one they share (pp_epilogue.h); this file keeps the persistent tile walk, the prefetch of the next tile's
// first K-step and bias / c1 / statistics rows, and the GEGLU epilogue.  Same packed
// weights, NHWC row layout and epilogue semantics as conv_gemm2.hip; launch_conv_gemm sends eligible shapes here (gemm_pp_config).
#include "common.h"
#include "conv_dispatch.h"
#include "conv_epilogue.h"
#include "pp_epilogue.h"
#include "pp_kloop.h"

namespace {

// GEGLU epilogue of the persistent ping-pong GEMM (TN = 4: a wave owns two packed (16 hidden | 16 gate) groups).  The weight rows are
// assigned to MFMA rows so that a lane holds, per 16-row tile, the hidden AND gate pre-activations of 8 consecutive output columns
// (fq * 8 .. + 7 of the wave's 32): 16-byte stores of the product and of both halves of the CF_GEGLU_RAW stash.  bias / c1 in packed order.
template <class MOf>
__device__ __forceinline__ void pp_epilogue_geglu(const ConvGemmParams& p, f32x4 (&acc)[8][4], MOf m_of, int wr, int wc, int n0,
                                                  const float* bias_s, const float* c1_s, int fr, int fq, const float* stats_s) {
  const int fl = p.flags;
  const int pk = wc * 64 + (fq >> 1) * 32 + (fq & 1) * 8;      // packed column (inside the tile) of this lane's first hidden value
  float4 bh[2], bg[2], ch[2], cg[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    bh[t] = *(const float4*)(bias_s + pk + t * 4); bg[t] = *(const float4*)(bias_s + pk + 16 + t * 4);
    ch[t] = *(const float4*)(c1_s + pk + t * 4); cg[t] = *(const float4*)(c1_s + pk + 16 + t * 4);
  }
  const int oc = (n0 >> 1) + wc * 32 + fq * 8;                  // output column of the lane's 8 products
#pragma unroll
  for (int a2 = 0; a2 < 8; a2 += 2) {
    float2 lst[2];
    int mrow[2];
#pragma unroll
    for (int a4 = 0; a4 < 2; ++a4) {
      mrow[a4] = m_of(wr * 128 + (a2 + a4) * 16 + fr);
      lst[a4] = (fl & CF_LNFOLD) ? *(const float2*)(stats_s + (wr * 128 + (a2 + a4) * 16 + fr) * 2) : make_float2(0.f, 1.f);
    }
#pragma unroll
    for (int a4 = 0; a4 < 2; ++a4) {
      const int a = a2 + a4, m = mrow[a4];
      const float rs = lst[a4].y * p.alpha, nm = -rs * lst[a4].x;      // alpha scales the folded term too: alpha * rstd * (acc - mean * c1) + b'
      float h[8], g[8];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float bhv[4] = {bh[t].x, bh[t].y, bh[t].z, bh[t].w}, bgv[4] = {bg[t].x, bg[t].y, bg[t].z, bg[t].w};
        const float chv[4] = {ch[t].x, ch[t].y, ch[t].z, ch[t].w}, cgv[4] = {cg[t].x, cg[t].y, cg[t].z, cg[t].w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          h[t * 4 + r] = __builtin_fmaf(rs, acc[a][2 * t][r], __builtin_fmaf(nm, chv[r], bhv[r]));
          g[t * 4 + r] = __builtin_fmaf(rs, acc[a][2 * t + 1][r], __builtin_fmaf(nm, cgv[r], bgv[r]));
        }
      }
      if (fl & CF_GEGLU_RAW) {
        bf16_t* rp = p.raw + (size_t)m * p.raw_ld + n0 + pk;
        *(uint4*)rp = pack8(h);
        *(uint4*)(rp + 16) = pack8(g);
      }
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = h[e] * gelu_f(g[e]);
      *(uint4*)((bf16_t*)p.y + (size_t)m * p.y_ld + oc) = pack8(o);
    }
  }
}

// The same ping-pong K loop for pointwise (1x1 / linear) layers, PERSISTENT: 256 x (64 TN) tiles, both operands streamed through two
// 64-deep stages (TN = 5: A 32 KB + W 40 KB per K-step, 6.9 B per kFLOP against 13.8 for the 128 x 160 two-workgroup form, every A
// row read once).  One workgroup per CU walks its share of the tiles (an XCD owns a contiguous range, n-tiles fastest, dealt round-robin
// to its workgroups); the first K-step of the NEXT tile (and its bias / c1 rows, 16-byte LDS-DMA pieces into a two-slot ring) is
// requested during the last K-step of the current one, so launch, prologue latency and the drain of the epilogue's stores no longer sit
// between two K loops (tools/pp_trace.py: 2.9 + 1.1 us of a 21 us tile at K = 320).  GEGLU: TN = 4 with the packed (hidden | gate) epilogue.
// ------------------------------------------------------------------------------------------------------------------------------------
#ifdef DD_TRACE
// debug build only (tools/pp_trace.py): per tile stamps in s_memrealtime ticks (10 ns) -- wait for the first K-step, K loop start, K loop
// end, end of the epilogue
__device__ unsigned long long g_pp_trace[8192 * 6];
#define PPS_STAMP(t, i) do { if (threadIdx.x == 0 && (t) < 8192) g_pp_trace[(t) * 6 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define PPS_STAMP(t, i) do { } while (0)
#endif
template <int TN, bool GEGLU>
__global__ __launch_bounds__(512, 1) void gemm_pps_kernel(ConvGemmParams p) {
  constexpr int BM = 256, BN = 4 * TN * 16;
  constexpr int BUF = (BM + BN) * 128;
  constexpr int NP = 4 + TN;                           // pieces per wave and K-step: 4 of A, TN of W
  constexpr int AUX = 2 * BUF;                         // [slot][bias 2 KB | c1 2 KB | (mean, rstd) of the tile's 256 rows 2 KB]
  constexpr int SLOT = 6144;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int fr = lane & 15, fq = lane >> 4;
  const int ntn = p.N / BN, tiles = (p.M / BM) * ntn;
  // this workgroup's tiles: first, first + per, ... (count of them) inside its XCD's contiguous range
  const int per = gridDim.x >> 3, slot = blockIdx.x >> 3;
  const XcdRange xr = xcd_tile_range(tiles, blockIdx.x);
  const int first = xr.first + slot, count = slot < xr.count ? (xr.count - slot + per - 1) / per : 0;
  if (count == 0) return;
  const int KT = p.K >> 6;
  const int prow = lane >> 3, j = (lane & 7) ^ prow;
  unsigned aoff[4], woff[TN];
#pragma unroll
  for (int i = 0; i < 4; ++i) aoff[i] = ((unsigned)((wave + 8 * i) * 8 + prow) * (unsigned)p.x_ld + (unsigned)(j * 8)) * 2u;
#pragma unroll
  for (int i = 0; i < TN; ++i)                           // MFMA-ordered row of the W stage -> weight row of the tile
    woff[i] = ((unsigned)pp_weight_row<TN, GEGLU>((wave + 8 * i) * 8 + prow) * (unsigned)p.K + (unsigned)(j * 8)) * 2u;
  // bias / c1 pieces of a tile: waves 0, 1 bring bias[n0 .. n0 + BN), waves 2, 3 c1 (256 floats per piece; absent rows read as zeros)
  const unsigned auxoff = (wave < 4 && (wave & 1) * 256 + lane * 4 < BN && ((wave < 2) ? (p.flags & CF_BIAS) : (p.flags & CF_LNFOLD)))
                              ? (unsigned)((wave & 1) * 256 + lane * 4) * 4u : 0xffffff00u;
  const float* auxbase = wave < 2 ? p.bias : p.ln_c1;
  // piece `which` of K-step kt of the tile at (xt, n0) into stage `buf`
  auto issue = [&](const bf16_t* xt, unsigned wsoff, int kt, int buf, int which) {
    unsigned char* b = smem + buf * BUF;
    if (which < 4) dma16(xt, b + (wave + 8 * which) * 1024, aoff[which], (unsigned)kt * 128u);
    else dma16(p.w, b + BM * 128 + (wave + 8 * (which - 4)) * 1024, woff[which - 4], wsoff + (unsigned)kt * 128u);
  };
  const unsigned statoff = (p.flags & CF_LNFOLD) ? (unsigned)((wave & 1) * 1024 + lane * 16) : 0xffffff00u;    // waves 4, 5: 128 rows x 8 B each
  auto issue_aux = [&](int m0, int n0, int slot) {
    if (wave < 4) dma16(auxbase ? (const void*)auxbase : (const void*)p.w, smem + AUX + slot * SLOT + (wave >> 1) * 2048 + (wave & 1) * 1024, auxoff, (unsigned)n0 * 4u);
    else if (wave < 6) dma16(p.ln_stats ? (const void*)(p.ln_stats + (size_t)m0 * 2) : (const void*)p.w, smem + AUX + slot * SLOT + 4096 + (wave & 1) * 1024, statoff, 0u);
  };
  int tile = first;
  int m0 = (tile / ntn) * BM, n0 = (tile % ntn) * BN;
  const bf16_t* xt = p.x + (size_t)m0 * p.x_ld;          // per-tile base: 32-bit byte offsets only span 256 rows
  unsigned wsoff = (unsigned)n0 * (unsigned)p.K * 2u;
  int cur = 0;
#pragma unroll
  for (int q = 0; q < NP; ++q) issue(xt, wsoff, 0, 0, q);
  issue_aux(m0, n0, 0);
  f32x4 acc[8][TN];
  for (int it = 0; it < count; ++it) {
    PPS_STAMP(tile, 0);
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
      for (int b = 0; b < TN; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    // next tile (wave-uniform)
    const bool have_next = it + 1 < count;
    const int tile_n = tile + per;
    const int m0n = (tile_n / ntn) * BM, n0n = (tile_n % ntn) * BN;
    const bf16_t* xtn = p.x + (size_t)m0n * p.x_ld;
    const unsigned wsoffn = (unsigned)n0n * (unsigned)p.K * 2u;
    // the first K-step of this tile was requested before the previous tile's epilogue (a counted wait that leaves the epilogue's last
    // stores in flight measured the same: what is left here is the skew between the eight waves' epilogues, tools/pp_trace.py)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    PPS_STAMP(tile, 1);
    if (wr == 1) __builtin_amdgcn_s_barrier();            // the lower row half runs one barrier behind
    for (int kt = 0; kt < KT; ++kt) {
      const unsigned char* Ab = smem + cur * BUF;
      const unsigned char* Bb = Ab + BM * 128;
      const bool more = kt + 1 < KT;
      const bool pre = more || have_next;
      const bf16_t* nx = more ? xt : xtn;
      const unsigned nw = more ? wsoff : wsoffn;
      const int nk = more ? kt + 1 : 0;
      // the last K-step leaves the next tile's first K-step in flight: only its LDS reads have to retire
      pp_kstep<TN>(acc, Bb, Ab, wc, fr, fq,
                   [&](int a) {
                     const int row = wr * 128 + a * 16 + fr;
                     return PpRow{row, row & 7};
                   },
                   [&] {
                     if (!pre) return;
#pragma unroll
                     for (int q = 0; q < NP; ++q) issue(nx, nw, nk, cur ^ 1, q);
                     if (!more) issue_aux(m0n, n0n, (it + 1) & 1);
                   },
                   more);
      cur ^= 1;
    }
    if (wr == 0) __builtin_amdgcn_s_barrier();
    PPS_STAMP(tile, 2);
    const float* bias_s = (const float*)(smem + AUX + (it & 1) * SLOT);
    const int m0c = m0;
    auto m_of = [&](int r) { return m0c + r; };
    auto sblk_of = [&](int r) { return (m0c + r) >> 6; };
    if constexpr (GEGLU) pp_epilogue_geglu(p, acc, m_of, wr, wc, n0, bias_s, bias_s + 512, fr, fq, bias_s + 1024);
    else pp_epilogue<TN>(p, acc, m_of, sblk_of, wr, wc, n0, bias_s, bias_s + 512, (n0 / BN) * 4 + wc, fr, fq, bias_s + 1024);
    PPS_STAMP(tile, 3);
    tile = tile_n; m0 = m0n; n0 = n0n; xt = xtn; wsoff = wsoffn;
  }
}

}  // namespace

// 0 = not eligible, else TN (5: 256 x 320 tiles; 4: 256 x 256 tiles of a GEGLU projection).  Epilogues: bias, residual, ReLU, CF_STATS,
// CF_ROWSTATS, CF_LNFOLD; GEGLU with bias, raw stash and CF_LNFOLD only
int gemm_pp_config(const ConvGemmParams& p) {
  constexpr int nmax = 3840;
  if (!conv_env().gemm_pp || p.force_small) return 0;
  if (p.ntaps != 1 || p.stride != 1 || p.shift || p.parity || p.H != p.Ho || p.W != p.Wo || (p.cin & 63) || p.K != p.cin) return 0;
  if ((p.M & 255) || p.K < 256 || p.ksplit > 1 || p.bias_sel || (p.x_ld & 7) || (p.y_ld & 7)) return 0;
  if ((size_t)256 * p.x_ld * 2 >= 0xF0000000ull || (size_t)p.N * p.K * 2 >= 0xF0000000ull) return 0;
  if (p.flags & CF_GEGLU) {
    if (!conv_env().gemm_pp_geglu) return 0;
    if (p.flags & ~(CF_BIAS | CF_GEGLU | CF_GEGLU_RAW | CF_LNFOLD)) return 0;
    if ((p.N & 255) || ((p.flags & CF_GEGLU_RAW) && (p.raw_ld & 7))) return 0;
    if ((p.M / 256) * (p.N / 256) < 192) return 0;
    return 4;
  }
  if (p.flags & ~(CF_BIAS | CF_RES | CF_RELU | CF_STATS | CF_ROWSTATS | CF_LNFOLD)) return 0;
  if (p.N % 320 || p.N > nmax) return 0;
  if ((p.flags & CF_RES) && (p.res_ld & 7)) return 0;
  if ((p.M / 256) * (p.N / 320) < 192) return 0;
  return 5;
}
// CF_ROWSTATS spans: one per wave of a 256 x 320 tile, 80 columns each
int gemm_pp_rowstat_spans(const ConvGemmParams& p) { return p.N / 80; }
template <int TN, bool GEGLU>
static hipError_t run_pps(const ConvGemmParams& p, hipStream_t stream) {
  constexpr int BN = 64 * TN;
  const int lds = 2 * (256 + BN) * 128 + 2 * 6144;
  static bool attr = false;
  if (!attr) { hipFuncSetAttribute((const void*)gemm_pps_kernel<TN, GEGLU>, hipFuncAttributeMaxDynamicSharedMemorySize, lds); attr = true; }
  const int cus = persistent_cus();
  const int tiles = (p.M / 256) * (p.N / BN);
  const int grid = tiles >= cus ? cus : (tiles + 7) & ~7;
  hipLaunchKernelGGL((gemm_pps_kernel<TN, GEGLU>), dim3(grid), dim3(512), lds, stream, p);
  return hipGetLastError();
}
hipError_t launch_gemm_pp(const ConvGemmParams& p, int tn, hipStream_t stream) {
  return tn == 4 ? run_pps<4, true>(p, stream) : run_pps<5, false>(p, stream);
}

#ifdef DD_TRACE
extern "C" int dd_debug_read_pp_trace(unsigned long long* host, int n) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_pp_trace), sizeof(unsigned long long) * n);
}
#endif
