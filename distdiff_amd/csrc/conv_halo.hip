// K1 (deep 3x3 shapes) -- implicit-GEMM 3x3 / stride-1 / pad-1 convolution (forward and input-gradient) with a HALO-resident input
// tile and a phase-alternating ("ping-pong") K loop, bf16 MFMA, gfx950.  Same packed weights, tap tables, NHWC row layout and epilogue
// semantics (bias / residual / ReLU / CF_STATS GroupNorm partials) as conv_gemm2.hip; launch_conv_gemm sends eligible shapes here.
//
// Why (profiles/r03_gemm_schedule_micro.txt): on a CU the LDS-DMA operand stream and the MFMA stream do not overlap
// to their individual rates -- a K-step costs about delivery time + MFMA time in every schedule tried -- so the lever is bytes per FLOP:
//   * the nine taps of a 64-channel chunk read the SAME input pixels shifted by (dy, dx): the tile's 256 output pixels (256 / W image
//     rows) plus a one-pixel border -- (R + 2) x (W + 2) pixels x 128 B -- are staged ONCE per chunk, zero-filled outside the image by
//     the buffer load's range check, and the A fragments of tap (dy, dx) are read at pixel + dy * (W + 2) + dx.  Input traffic per
//     K-step falls from 32 KB to ~5.6 KB; only the weights stream every K-step;
//   * 512 x 160 / 512 x 128 / 256 x 320 / 256 x 256 tiles, 8 waves as 4 x 2 or 2 x 4, wave tile 128 x 80 (64): 20-40 KB of weights per
//     10.5 MFLOP K-step;
//   * the two waves of a SIMD (different row groups) run the same program one s_barrier apart: between two barriers one issues the
//     8 * TN MFMAs of a K half while the other reads fragments and issues its share of the next K-step's weight DMA
//     (cdna_hip_programming.md section 5, "The 256^2 8-phase template"; MI355X_MICROARCH.md "Two waves per SIMD").
// The 3x3 kernel is not persistent (one workgroup per tile, XCD-aware tile order, n-tiles fastest inside an XCD: a persistent form
// measured slower); the pointwise GEMM of the same loop (gemm_pps_kernel, gemm_pps.hip) is.
// Where the loop lives: pp_kloop.h holds the K-step (pp_kstep, also gemm_pps_kernel's), the chunk x tap loop around it with the halo refill
// (pp_halo_kloop, called by both kernels of this file) and the weight-row map (pp_weight_row); pp_epilogue.h the epilogue; common.h the XCD
// tile range.  This file keeps what differs between its two kernels: tile selection and the persistent walk, the two halo address schemes,
// the prologues, the narrow and chunk-split stores.  Stating the rest of the device side once for both kernels (LDS layout, thread
// decomposition, tile context, halo pixel split, one refill stager) kept registers, scratch and bits but measured 1-3 % slower in every
// instantiation, so the kernels keep their own text (profiles/halo_unified.json).
// Host side, at the end of the file: halo_geometry, conv_halo_plan (the ONE decision: form, kernel, chunk split, address table, LDS bytes,
// grid) and launch_conv_halo, which acts on that plan and recomputes nothing.
#include "common.h"
#include "conv_dispatch.h"
#include "conv_epilogue.h"
#include "pp_epilogue.h"
#include "pp_kloop.h"

namespace {

// (Tile geometry: HaloGeo, conv_dispatch.h; host: halo_geometry.)
// CF_STATS block slot of the 64 tile pixels r .. r + 63 (r % 64 == 0) of the tile at (y0, x0) of the image whose first output row is mimg.
// tw >= 64: they are 64 consecutive output rows m inside one image row, slot m >> 6 as in every other kernel.  tw = 16 / 32: they are
// 64 / tw image rows x tw pixels, which with several tiles per image row are NOT consecutive in m; the consumer (norm.hip,
// gn_finalize_chan_kernel) merges the Ho * Wo / 64 slots of an image as an unordered set of equal-count (64) partials, so any one-to-one
// map of the image's 64-pixel groups onto its slots is correct: slot = (row group) * tiles_x + (tile column).  Row groups are whole
// (th is a multiple of 64 / tw), so the map is one-to-one; with one tile per image row it is m >> 6 again.
__device__ __forceinline__ int halo_stats_block(int mimg, int y0, int x0, int r, int lw, int Wo, int tiles_x) {
  if (lw >= 6) return (mimg + (y0 + (r >> lw)) * Wo + x0 + (r & ((1 << lw) - 1))) >> 6;
  return (mimg >> 6) + ((y0 + (r >> lw)) >> (6 - lw)) * tiles_x + (x0 >> lw);
}

// WN = 4: 256 x (64 TN) tiles, waves 2 (M) x 4 (N); WN = 2: 512 x (32 TN) tiles, waves 4 (M) x 2 (N) -- the narrow outputs of the decoder's
// last level (N = 128).  Either way a wave owns 128 rows x TN * 16 columns and waves w, w + 4 (one SIMD) sit in different row groups.
// MI: the 8 x 8 level's form -- multi-image tiles + chunk split with fp32 partial sums; its own instantiation so that the hot forms
// keep their register allocation (as runtime branches the additions took the TN = 5 kernels from 12 to 80 bytes of scratch).
template <int TN, int WN, bool MI = false>
__global__ __launch_bounds__(512, 1) void conv_halo_kernel(ConvGemmParams p, HaloGeo geo) {
  const int lw = geo.ltw, halo_px = geo.halo_px;
  constexpr int BM = (8 / WN) * 128, BN = WN * TN * 16;
  constexpr int NPC = BN / 8;                           // weight pieces (8 rows x 128 B) per K-step
  constexpr int NWP = (NPC + 7) / 8;                    // ... per wave (the last one only on the first NPC % 8 waves when BN % 64 != 0)
  constexpr int WB = BN * 128;                          // bytes of one weight stage
  constexpr unsigned OOB = 0xfffffff0u;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* const halo = smem + 2 * WB;
  float* const bias_s = (float*)(halo + ((halo_px + 7) & ~7) * 128);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave / WN, wc = wave % WN;
  const int grp = wave >> 2;                            // SIMD partners w, w + 4 are in different groups: group 1 runs one barrier behind
  const int fr = lane & 15, fq = lane >> 4;
  const int Wd = 1 << lw, W2 = Wd + 2;

  // ---- tile of this workgroup (n-tiles fastest; blocks b, b + 8, ... share an XCD)
  const int ntn = (p.N + BN - 1) / BN, tiles = (p.M / BM) * ntn;      // (N < BN: the narrow form TN = 1, one n-tile)
  const int tile = xcd_tile_range(tiles, blockIdx.x).first + (blockIdx.x >> 3);
  const int n0 = (tile % ntn) * BN;
  const int mt = tile / ntn, tpi = geo.tiles_x * geo.tiles_y;
  const int ipt = MI ? geo.ipt : 1;                       // > 1: the tile is ipt whole (8 x 8) images, output rows contiguous
  const int img = MI ? mt * ipt : mt / tpi, tin = MI ? 0 : mt - img * tpi;
  const int y0 = (tin / geo.tiles_x) * geo.th, x0 = (tin % geo.tiles_x) << lw;    // first output pixel of the tile inside its image
  const int himg = MI ? (geo.th + 2) * W2 : 0;            // halo pixels of one image of a multi-image tile
  const int kz = MI ? blockIdx.y : 0;                     // chunk split (8 x 8 level: too few tiles to fill the chip): fp32 partial sums
  const int mimg = img * p.Ho * p.Wo;
  auto m_of = [&](int r) { return mimg + (y0 + (r >> lw)) * p.Wo + x0 + (r & (Wd - 1)); };   // output row of tile pixel r
  auto sblk_of = [&](int r) { return halo_stats_block(mimg, y0, x0, r, lw, p.Wo, geo.tiles_x); };
  const int chunks_all = p.cin >> 6;
  const int cper = MI ? (chunks_all + p.ksplit - 1) / (p.ksplit > 0 ? p.ksplit : 1) : chunks_all;
  const int c_begin = MI ? kz * cper : 0, c_end = MI ? min(chunks_all, c_begin + cper) : chunks_all;

  // ---- per-tap offsets: lane t holds tap t ((dy + 32) << 6 | (dx + 32)); read with readlane where needed
  const int v_taps = lane < 9 ? p.taptab[lane] : 0;
  if (tid < BN) bias_s[tid] = ((p.flags & CF_BIAS) && n0 + tid < p.N) ? p.bias[n0 + tid] : 0.f;

  // ---- weight staging: wave w moves pieces w, w + 8, ... (8 rows x 128 B) of the BN weight rows of a K-step.  LDS row R of a wave's
  // TN * 16 span holds output channel pp_weight_row(R).
  const int prow = lane >> 3, jw = (lane & 7) ^ prow;
  unsigned woff[NWP];
#pragma unroll
  for (int i = 0; i < NWP; ++i) {
    const int R = (wave + 8 * i) * 8 + prow, ch = pp_weight_row<TN>(R);
    // (rows behind the last output channel -- the narrow form pads N = 3 / 4 to a 32-row stage -- read as zeros: out of range)
    woff[i] = (((NPC & 7) == 0 || R < BN) && n0 + ch < p.N) ? ((unsigned)(n0 + ch) * (unsigned)p.K + (unsigned)(jw * 8)) * 2u : OOB;
  }
  auto issue_w = [&](int kt) {                           // this wave's pieces of K-step kt into its stage
#pragma unroll
    for (int i = 0; i < NWP; ++i)
      if ((NPC & 7) == 0 || wave + 8 * i < NPC) dma16(p.w, smem + (kt & 1) * WB + (wave + 8 * i) * 1024, woff[i], (unsigned)(c_begin * 9 + kt) * 128u);
  };
  // ---- halo staging (row half 0 only): pieces wave, wave + 4, ... of ceil(halo_px / 8); a lane's pixel hp = 8 * piece + (lane >> 3)
  const float inv_w2 = 1.f / (float)W2;
  const bf16_t* ximg = p.x + (size_t)img * p.H * p.W * p.x_ld;     // per-image base: 32-bit byte offsets only span one image
  // Halo address table (geo.tab; see 3.8.8 of DESIGN.md and conv_halo_persist_kernel): a workgroup of this kernel has ONE tile, so the byte
  // offset of every (piece, lane) of its halo -- out-of-image pixels as the out-of-range offset that reads zeros -- is the same for every
  // chunk.  All 8 waves compute their pieces once, in the prologue, store them behind the bias block and request chunk c_begin with
  // them; the refills at the chunk boundaries (row group 0) are a table read + a request per piece.
  unsigned* const htab = (unsigned*)(bias_s + BN);
  const bool use_tab = geo.tab != 0;
  auto halo_voff = [&](int pc) {
    const int hp = pc * 8 + prow;
    const int hi = MI ? (int)(((float)hp + 0.5f) * (1.f / (float)(himg > 0 ? himg : 1))) : 0;    // image of the tile
    const int hq = hp - hi * himg;
    const int hy = (int)(((float)hq + 0.5f) * inv_w2), hx = hq - hy * W2;
    const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;       // logical input pixel (= output pixel coordinates: stride 1, pad 1)
    const bool ok = hp < halo_px && iy >= 0 && iy < p.Ho && ix >= 0 && ix < p.Wo;
    const int j = (lane & 7) ^ (hx & 7);
    return ok ? ((unsigned)(hi * p.H * p.W + (iy >> p.shift) * p.W + (ix >> p.shift)) * (unsigned)p.x_ld + (unsigned)(j * 8)) * 2u : OOB;
  };
  auto first_halo = [&](int chunk) {                     // prologue, all 8 waves
    const int npc = (halo_px + 7) >> 3;
    for (int pc = wave; pc < npc; pc += 8) {
      const unsigned voff = halo_voff(pc);
      htab[pc * 64 + lane] = voff;
      dma16(ximg, halo + pc * 1024, voff, (unsigned)chunk * 128u);
    }
  };
  auto issue_halo = [&](int chunk) {                     // row group 0 (waves 0 .. 3)
    const int npc = (halo_px + 7) >> 3;
    const unsigned soff = (unsigned)chunk * 128u;
    if (use_tab) {
      for (int pc = wave; pc < npc; pc += 16) {         // four pieces per round: table reads first, then the requests back to back
        unsigned e[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) e[u] = pc + 4 * u < npc ? htab[(pc + 4 * u) * 64 + lane] : OOB;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (pc + 4 * u >= npc) break;
          dma16(ximg, halo + (pc + 4 * u) * 1024, e[u], soff);
        }
      }
      return;
    }
    for (int pc = wave; pc < npc; pc += 4) dma16(ximg, halo + pc * 1024, halo_voff(pc), soff);
  };

  f32x4 acc[8][TN];
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- prologue
  if (use_tab) first_halo(c_begin);
  else if (grp == 0) issue_halo(c_begin);
  issue_w(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();                                      // also publishes bias_s
  if (grp == 1) __builtin_amdgcn_s_barrier();           // the second group runs one barrier behind
  pp_halo_kloop<TN, WB, MI>(acc, smem, halo, c_begin, c_end, 0, v_taps, lw, grp, wr, wc, fr, fq, issue_halo, issue_w);
  if (grp == 0) __builtin_amdgcn_s_barrier();           // balance the barrier count of the two groups

  if constexpr (MI) {
    // chunk split: raw fp32 partial sums [split][M][N]; splitk_reduce_kernel adds them and applies the epilogue
    constexpr int TNP2 = TN & ~1;
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      float* pr = p.partial + ((size_t)kz * p.M + m_of(wr * 128 + a * 16 + fr)) * p.N + n0 + wc * (TN * 16);
#pragma unroll
      for (int jn = 0; jn < TN; ++jn) {
        const int col = jn < TNP2 ? (jn >> 1) * 32 + fq * 8 + (jn & 1) * 4 : jn * 16 + fq * 4;
        *(float4*)(pr + col) = make_float4(acc[a][jn][0], acc[a][jn][1], acc[a][jn][2], acc[a][jn][3]);
      }
    }
    return;
  }
  if constexpr (TN == 1) {
    // narrow form (conv_out: N <= 4): channels 0 .. 3 of a pixel are the four accumulator rows of lane group 0 of the first column wave;
    // bias only; fp32 (CF_OUT_F32: the image / eps rows are 8 floats wide and only the N valid ones may be written) or bf16 output
    if (wc == 0 && fq == 0) {
      const float4 b4 = *(const float4*)bias_s;
#pragma unroll
      for (int a = 0; a < 8; ++a) {
        const int m = m_of(wr * 128 + a * 16 + fr);
        const float v[4] = {acc[a][0][0] + b4.x, acc[a][0][1] + b4.y, acc[a][0][2] + b4.z, acc[a][0][3] + b4.w};
        if (p.flags & CF_OUT_F32) {
          float* yp = (float*)p.y + (size_t)m * p.y_ld;
          if (p.N == 4) *(float4*)yp = make_float4(v[0], v[1], v[2], v[3]);
          else
#pragma unroll
            for (int r = 0; r < 4; ++r) if (r < p.N) yp[r] = v[r];
        } else {
          bf16_t* yp = (bf16_t*)p.y + (size_t)m * p.y_ld;
#pragma unroll
          for (int r = 0; r < 4; ++r) if (r < p.N) yp[r] = f2bf(v[r]);
        }
      }
    }
  } else {
    pp_epilogue<TN>(p, acc, m_of, sblk_of, wr, wc, n0, bias_s, bias_s, 0, fr, fq);
  }
}

#ifdef DD_TRACE
// debug build only (tools/halo_trace.py): per tile stamps in s_memrealtime ticks (10 ns)
__device__ unsigned long long g_halo_trace[8192 * 6];
#define HP_STAMP(t, i) do { if (threadIdx.x == 0 && (t) < 8192) g_halo_trace[(t) * 6 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define HP_STAMP(t, i) do { } while (0)
#endif
// PERSISTENT form of the halo kernel for the tile shapes whose K loop is short (the decoder's levels: Cin = 128 / 256 / 512, i.e. 18 / 36 /
// 72 K-steps per 512 x 128 tile).  There a tile's prologue (100 KB of halo + the first weight stage: DMA issue, flight and drain with
// nothing beside them) and its epilogue (128 KB of stores + the GroupNorm partials) are a quarter of the tile, and with one workgroup per
// CU (LDS) nothing overlaps them.  One workgroup per CU walks its tiles: behind the last K-step of a tile the halo buffer and the idle
// weight stage are free, so the NEXT tile's first halo chunk, first weight stage and bias row are requested BEFORE this tile's epilogue
// and land while it stores.  Same tile -> XCD map as the one-tile kernel (an XCD's workgroups share a contiguous tile range, n-tiles
// fastest), the same K loop (pp_halo_kloop) and epilogue (pp_epilogue); N % BN == 0.  Results are bitwise those of conv_halo_kernel
// (same order of operations per tile; tests/test_pingpong_bits_gpu.py).
template <int TN, int WN>
__global__ __launch_bounds__(512, 1) void conv_halo_persist_kernel(ConvGemmParams p, HaloGeo geo) {
  const int lw = geo.ltw, halo_px = geo.halo_px;
  constexpr int BM = (8 / WN) * 128, BN = WN * TN * 16;
  constexpr int NPC = BN / 8, NWP = (NPC + 7) / 8, WB = BN * 128;
  static_assert((NPC & 7) == 0, "whole weight pieces per wave");
  constexpr unsigned OOB = 0xfffffff0u;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* const halo = smem + 2 * WB;
  float* const bias_base = (float*)(halo + ((halo_px + 7) & ~7) * 128);      // two slots of BN floats (tile parity)

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave / WN, wc = wave % WN;
  const int grp = wave >> 2;
  const int fr = lane & 15, fq = lane >> 4;
  const int Wd = 1 << lw, W2 = Wd + 2;
  const int ntn = p.N / BN, tiles = (p.M / BM) * ntn, tpi = geo.tiles_x * geo.tiles_y;
  // tiles of this workgroup: XCD x owns [xs, xs + xc); its gridDim.x / 8 workgroups take xs + idx, xs + idx + per, ...
  const int per = gridDim.x >> 3;
  const XcdRange xr = xcd_tile_range(tiles, blockIdx.x);
  const int xs = xr.first, xc = xr.count;
  int t = blockIdx.x >> 3;
  if (t >= xc) return;
  const int chunks = p.cin >> 6, KT = chunks * 9;
  const int v_taps = lane < 9 ? p.taptab[lane] : 0;
  const int prow = lane >> 3, jw = (lane & 7) ^ prow;
  unsigned woff[NWP];                                   // lane part of the weight offsets (n0 goes into the scalar offset)
#pragma unroll
  for (int i = 0; i < NWP; ++i)
    woff[i] = ((unsigned)pp_weight_row<TN>((wave + 8 * i) * 8 + prow) * (unsigned)p.K + (unsigned)(jw * 8)) * 2u;
  const float inv_w2 = 1.f / (float)W2;
  // ---- halo address table (LDS, built once per workgroup): the LDS-DMA requests of a halo refill were bound by their ADDRESS ARITHMETIC
  // (~35 instructions and two divergent branches per 1 KB piece: ~210 cycles a piece, 2.5 us per refill with cache-hot data as with cold,
  // profiles/r06_decoder_persist.txt), and everything in it but the tile's origin is the same for every tile and chunk.  Entry (piece,
  // lane) = halo row (5 bits) | halo column (8 bits) | byte offset from the halo's first pixel / 16 (19 bits, swizzle included); per
  // tile only the origin pointer and the range of rows / columns that lie inside the image change (scalars).
  unsigned* const htab = (unsigned*)(bias_base + 2 * BN);
  const int npc = (halo_px + 7) >> 3;
  for (int pc = wave; pc < npc; pc += 8) {
    const int hp = pc * 8 + prow;
    const int hy = (int)(((float)hp + 0.5f) * inv_w2), hx = hp - hy * W2;
    const int sy = p.shift ? (hy + 1) >> 1 : hy, sx = p.shift ? (hx + 1) >> 1 : hx;     // stored pixel relative to the halo's first one
    const int j = (lane & 7) ^ (hx & 7);
    const unsigned rel = ((unsigned)(sy * p.W + sx) * (unsigned)p.x_ld + (unsigned)(j * 8)) * 2u;
    htab[pc * 64 + lane] = hp < halo_px ? ((unsigned)hy << 27) | ((unsigned)hx << 19) | (rel >> 4) : 0xf8000000u;    // row 31: never inside
  }
  struct Tile { int n0, img, y0, x0; };
  auto tile_of = [&](int tt) {
    const int tile = xs + tt;
    Tile g;
    g.n0 = (tile % ntn) * BN;
    const int mt = tile / ntn;
    g.img = mt / tpi;
    const int tin = mt - g.img * tpi;
    g.y0 = (tin / geo.tiles_x) * geo.th; g.x0 = (tin % geo.tiles_x) << lw;
    return g;
  };
  // this wave's pieces of weight K-step kt of tile g into stage st
  auto issue_w = [&](const Tile& g, int kt, int st) {
#pragma unroll
    for (int i = 0; i < NWP; ++i)
      dma16(p.w, smem + st * WB + (wave + 8 * i) * 1024, woff[i], (unsigned)g.n0 * (unsigned)p.K * 2u + (unsigned)kt * 128u);
  };
  auto issue_halo = [&](const Tile& g, int chunk, int nw) {     // nw = 4: waves 0 .. 3 (refill inside the K loop); 8: all waves (between tiles)
    // first stored pixel of the halo (logical (y0 - 1, x0 - 1); may lie in front of the image: those lanes are masked below)
    const int oy = p.shift ? (g.y0 >> 1) - 1 : g.y0 - 1, ox = p.shift ? (g.x0 >> 1) - 1 : g.x0 - 1;
    const bf16_t* xo = p.x + ((long long)g.img * p.H * p.W + (long long)oy * p.W + ox) * p.x_ld;
    // halo rows / columns inside the image: logical pixel y0 - 1 + hy in [0, Ho)
    const unsigned ylo = (unsigned)max(0, 1 - g.y0), yn = (unsigned)min(geo.th + 2, p.Ho - g.y0 + 1) - ylo;
    const unsigned xlo = (unsigned)max(0, 1 - g.x0), xn = (unsigned)min(Wd + 2, p.Wo - g.x0 + 1) - xlo;
    const unsigned soff = (unsigned)chunk * 128u;
    for (int pc = wave; pc < npc; pc += 4 * nw) {       // four pieces per round: table reads first, then the requests back to back
      unsigned e[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) e[u] = pc + nw * u < npc ? htab[(pc + nw * u) * 64 + lane] : 0xf8000000u;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (pc + nw * u >= npc) break;
        const bool ok = ((e[u] >> 27) - ylo) < yn && (((e[u] >> 19) & 255u) - xlo) < xn;
        dma16(xo, halo + (pc + nw * u) * 1024, ok ? (e[u] & 0x7ffffu) << 4 : OOB, soff);
      }
    }
  };
  auto stage_first = [&](const Tile& g, int st, int slot) {   // everything a tile needs before its first K-step (all waves are between tiles here)
    issue_halo(g, 0, 8);
    issue_w(g, 0, st);
    if (tid < BN) bias_base[slot * BN + tid] = (p.flags & CF_BIAS) ? p.bias[g.n0 + tid] : 0.f;
  };

  Tile g = tile_of(t);
  int kg = 0;                                             // K-steps issued so far: K-step kt of the current tile lives in stage (kg + kt) & 1
  __syncthreads();                                      // the address table is complete
  stage_first(g, 0, 0);
  for (int it = 0;; ++it) {
    HP_STAMP(xs + t, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                    // halo chunk 0, weight stage, bias slot of this tile are in LDS
    HP_STAMP(xs + t, 1);
    if (grp == 1) __builtin_amdgcn_s_barrier();         // the second group runs one barrier behind
    f32x4 acc[8][TN];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
      for (int b = 0; b < TN; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    pp_halo_kloop<TN, WB, false>(acc, smem, halo, 0, chunks, kg, v_taps, lw, grp, wr, wc, fr, fq,
                                 [&](int c) { issue_halo(g, c, 4); }, [&](int kt) { issue_w(g, kt, (kg + kt) & 1); });
    if (grp == 0) __builtin_amdgcn_s_barrier();         // balance the barrier count of the two groups: every LDS read of this tile has retired
    HP_STAMP(xs + t, 2);
    kg += KT;
    const int tn_ = t + per;
    const bool have_next = tn_ < xc;
    Tile gn = g;
    if (have_next) {
      gn = tile_of(tn_);
      stage_first(gn, kg & 1, (it + 1) & 1);            // lands under the epilogue below
    }
    HP_STAMP(xs + t, 3);
    const int mimg = g.img * p.Ho * p.Wo, y0 = g.y0, x0 = g.x0;
    auto m_of = [&](int r) { return mimg + (y0 + (r >> lw)) * p.Wo + x0 + (r & (Wd - 1)); };
    const float* bias_s = bias_base + (it & 1) * BN;
    // look-ahead 2: 4 measured 2-3 % SLOWER on every decoder shape (256 VGPRs + 10 spills; profiles/r06_decoder_persist.txt)
    auto sblk_of = [&](int r) { return halo_stats_block(mimg, y0, x0, r, lw, p.Wo, geo.tiles_x); };
    pp_epilogue<TN, 2>(p, acc, m_of, sblk_of, wr, wc, g.n0, bias_s, bias_s, 0, fr, fq);
    HP_STAMP(xs + t, 4);
    if (!have_next) break;
    g = gn; t = tn_;
  }
}

// ---- the host side: geometry, the one plan, the one launch --------------------------------------------------------------------------------
bool halo_geometry(const ConvGemmParams& p, int bm, HaloGeo* g) {
  const int Wo = p.Wo, Ho = p.Ho;
  g->ipt = 1;
  if (Wo == 8 && Ho == 8 && bm == 256 && p.B % 4 == 0 && !p.shift) {
    // 8 x 8 level: a 256-pixel tile is four whole images, each with its own 10 x 10 halo block
    g->ltw = 3; g->th = 8; g->halo_px = 4 * 100; g->tiles_x = 1; g->tiles_y = 1; g->ipt = 4; g->tab = 0;
    return true;
  }
  // Tile width tw: the largest power-of-two factor of Wo, capped -- 512-pixel tiles are 8 rows x 64 pixels (halo 10 x 66 = 660 pixels) rather
  // than 4 x 128 (6 x 130 = 780): the halo refill at every 64-channel chunk boundary is the largest exposed cost of the decoder's short
  // K loops (tools/halo_trace.py: ~5 us of a 14.6 us chunk), and it scales with the halo's bytes; 256-pixel tiles are at most 128 wide.
  // A power-of-two Wo gives what it always gave (Wo itself below 128, else 64 / 128); 96 -> 32 (3 tiles per row), 48 / 80 -> 16,
  // 160 -> 32, 192 / 320 -> 64, 384 / 640 / 768 -> 64 or 128.  tw >= 16 is what the kernels' LDS swizzle needs (16-pixel MFMA row tiles
  // start at multiples of 16 inside a tile row): widths whose power-of-two factor is 8 or less (24, 12, 40, 20, 10) stay on the general
  // kernels, and the 8 x 8 multi-image form above is the only narrower one.  th = bm / tw is a power of two >= 2, so every tile origin
  // (y0, x0) is even: the fused-upsample forms (p.shift = 1) rely on it for (y0 - 1 + hy) >> 1 == (y0 >> 1) - 1 + ((hy + 1) >> 1).
  // CF_STATS with tw < 64 and several tiles per row: halo_stats_block.
  const int cap = bm == 512 ? 64 : 128;
  int tw = Wo & -Wo;
  if (tw > cap) tw = cap;
  if (tw < 16) return false;
  const int th = bm / tw;
  if (th < 2 || (th & 1) || th > Ho || Ho % th) return false;
  int l = 0;
  while ((1 << l) < tw) ++l;
  g->ltw = l; g->th = th; g->halo_px = (th + 2) * (tw + 2); g->tiles_x = Wo / tw; g->tiles_y = Ho / th;
  g->tab = 0;
  return true;
}

constexpr int LDS_MAX = 163840;
// Dynamic LDS of a form with bn columns on a halo of halo_px pixels, as the kernels carve it: two weight stages, the halo (whole 8-pixel
// pieces), the bias row (persistent kernel: two slots, tile parity), the halo address table (persistent kernel: always; one-tile: table)
struct HaloLds {
  int plain, table_bytes;
  constexpr int total(bool with_table) const { return plain + (with_table ? table_bytes : 0); }
};
constexpr HaloLds halo_lds(int bn, int halo_px, bool persist) {
  return {2 * bn * 128 + ((halo_px + 7) & ~7) * 128 + (persist ? 2 : 1) * bn * 4 + 64, ((halo_px + 7) >> 3) * 256};
}

// chunk split of the 8 x 8 level (M = 64 pixels x images: 64 tiles of 256 x 320 at 64 images -- a quarter of the chip): the smallest
// power of two that gives >= 192 workgroups -- halved until it DIVIDES the chunk count (the kernel hands ceil(chunks / split) chunks to
// every blockIdx.y: with a remainder the last workgroups would start behind the last chunk; Cin = 2560 at 16 images: 16 -> 8) -- with
// every workgroup >= 2 chunks; 1 = this is not that case.  Needs the split-K scratch, large enough for the split's fp32 partial sums.
int halo_chunk_split(const ConvGemmParams& p, size_t partial_cap_bytes) {
  if (!conv_env().halo_8x8 || p.Wo != 8 || p.Ho != 8 || p.H != 8 || p.W != 8 || p.shift || p.stride != 1 || (p.B & 3) || p.N % 320 || !p.partial) return 1;
  if (p.flags & ~(CF_BIAS | CF_RES | CF_RELU)) return 1;
  const int tiles = (p.M / 256) * (p.N / 320), chunks = p.cin >> 6;
  int s = 1;
  while (tiles * s < 192 && s < 16) s *= 2;
  while (s > 1 && (chunks % s || chunks / s < 2)) s >>= 1;
  return (size_t)s * p.M * p.N * sizeof(float) > partial_cap_bytes ? 1 : s;      // scratch too small: no split form
}

// Form f on this problem, or false: geometry, kernel, address table, LDS bytes and grid -- each decided here and nowhere else.  split > 1:
// the chunk-split form of the 8 x 8 level, the only one whose tiles are four whole images and that need not fill the chip by tiles alone.
bool halo_plan_form(const ConvGemmParams& p, const HaloForm& f, int split, HaloPlan* hp) {
  const ConvEnv& env = conv_env();
  HaloGeo g;
  if (!halo_geometry(p, f.bm(), &g) || (g.ipt > 1) != (f.multi_image && split > 1)) return false;
  const int tiles = (p.M / f.bm()) * ((p.N + f.bn() - 1) / f.bn());       // (N < bn: the narrow form, one n-tile)
  if (split == 1 && tiles < 192) return false;            // needs (most of) the chip: small grids keep the split-K forms
  const HaloLds one = halo_lds(f.bn(), g.halo_px, false), per = halo_lds(f.bn(), g.halo_px, true);
  if (one.total(false) > LDS_MAX) return false;
  // conv_halo_persist_kernel: 512 x 128 tiles with a short K loop (the decoder's levels, any width halo_geometry accepts: 128 ... 1024
  // as 192 / 384 / 768), next tile's first stage requested under the epilogue.  Its address table: p.shift <= 1 ((hy + 1) >> 1), halo
  // row < 31, column < 256, byte offsets inside the halo's stored rows below 8 MB.
  const bool persist = f.persist && env.halo_persist && p.shift <= 1 && g.ipt == 1 && p.N % f.bn() == 0 && (p.cin >> 6) <= env.halo_persist * 8 &&
                       g.th + 2 < 31 && (1 << g.ltw) + 2 < 256 && (size_t)(g.th + 3) * p.W * p.x_ld * 2 < (8u << 20) && per.total(true) <= LDS_MAX;
  g.tab = persist || (env.halo_tab && one.total(true) <= LDS_MAX);        // the one-tile kernel: behind the bias block when it fits
  const int cus = persistent_cus();
  *hp = HaloPlan{f.id, persist ? KIND_HALO_PERSIST : KIND_HALO, split, g, persist ? per.total(true) : one.total(g.tab != 0),
                 persist ? (tiles >= cus ? cus : (tiles + 7) & ~7) : tiles, split};
  return true;
}

// the instantiation that runs a plan, by the names of HALO_FORMS.  attr: the dynamic LDS bytes fn has been raised to
struct HaloEntry { int form, kind; bool multi_image; void (*fn)(ConvGemmParams, HaloGeo); int attr; };
template <int ID, bool MI = false>
constexpr HaloEntry one_tile() { constexpr HaloForm f = halo_form(ID); return {ID, KIND_HALO, MI, conv_halo_kernel<f.tn, f.wn, MI>, 0}; }
template <int ID>
constexpr HaloEntry persistent() { constexpr HaloForm f = halo_form(ID); return {ID, KIND_HALO_PERSIST, false, conv_halo_persist_kernel<f.tn, f.wn>, 0}; }

}  // namespace

// The plan of a halo launch, or false (not eligible: shape, flags, alignment, 32-bit offsets, no form fits).  Epilogues: bias, residual,
// ReLU, CF_STATS (the narrow form: bias, fp32 output).  The host reads the tap table once per weight tensor elsewhere: here the caller
// guarantees a 3x3 / pad 1 table (ntaps == 9 with offsets in {-1, 0, 1}^2), which every packer emits for KH = KW = 3, pad = 1.
bool conv_halo_plan(const ConvGemmParams& p, size_t partial_cap_bytes, HaloPlan* hp) {
  const ConvEnv& env = conv_env();
  if (!env.conv_halo || p.force_small) return false;
  if (p.ntaps != 9 || p.stride != 1 || p.shift > 1 || p.parity || (p.H << p.shift) != p.Ho || (p.W << p.shift) != p.Wo || (p.cin & 63) ||
      p.K != 9 * p.cin) return false;
  // narrow outputs (conv_out of the decoder / the UNet, N <= 4): a 512 x 32 form whose weight stage is 4 KB -- the input tile is read once
  // from HBM (halo) instead of being gathered tap by tap through the 128-wide tiles of the general kernels (60 of 64 columns wasted)
  const bool narrow = env.halo_narrow && p.N <= 4 && !(p.flags & ~(CF_BIAS | CF_OUT_F32)) && !p.bias_sel && !p.shift && p.ksplit <= 1;
  if (!narrow && ((p.flags & ~(CF_BIAS | CF_RES | CF_RELU | CF_STATS)) || p.bias_sel)) return false;
  if ((!narrow && (p.y_ld & 7)) || ((p.flags & CF_RES) && (p.res_ld & 7)) || (p.x_ld & 7) || p.alpha != 1.f) return false;
  if ((size_t)p.H * p.W * (size_t)p.x_ld * 2 >= 0xF0000000ull) return false;     // byte offsets are per image
  if (p.M != p.B * p.Ho * p.Wo) return false;
  if (narrow) {
    if (p.N == 4 && (p.flags & CF_OUT_F32) && (p.y_ld & 3)) return false;         // float4 stores
    return halo_plan_form(p, halo_form(HALO_NARROW), 1, hp);
  }
  // 8 x 8 level: 256 x 320 multi-image tiles + chunk split (fp32 partials into the split-K scratch, then the reduce kernel)
  const int split = halo_chunk_split(p, partial_cap_bytes);
  if (split > 1) return halo_plan_form(p, halo_form(HALO_256x320), split, hp);
  if (p.ksplit > 1) return false;
  // tile forms by preference: 512 x 160 / 512 x 128 (20 / 16 KB of weights + ~10 KB of halo per K-step instead of 40 / 32 + 5.6) where the
  // image geometry allows 512-pixel tiles, else 256 x 320 / 256 x 256
  for (const HaloForm& f : HALO_FORMS) {
    if (f.id == HALO_NARROW || p.N % f.bn()) continue;
    if (f.bm() == 512 && !env.halo_tall && p.N != 128) continue;
    if (f.bn() == 128 && p.N % 320 == 0) continue;      // 320-multiples: 160-wide tiles
    if (halo_plan_form(p, f, 1, hp)) return true;
  }
  return false;
}

// Raises the kernel's dynamic LDS limit where needed and launches the plan, for both kernels.  p.ksplit = hp.split (the planner sets it).
hipError_t launch_conv_halo(const ConvGemmParams& p, const HaloPlan& hp, hipStream_t stream) {
  static HaloEntry entries[] = {persistent<HALO_512x128>(), one_tile<HALO_NARROW>(), one_tile<HALO_512x128>(), one_tile<HALO_256x256>(),
                                one_tile<HALO_256x320>(), one_tile<HALO_256x320, true>(), one_tile<HALO_512x160>()};
  for (HaloEntry& e : entries) {
    if (e.form != hp.form || e.kind != hp.kind || e.multi_image != (hp.geo.ipt > 1)) continue;
    if (e.attr < hp.lds) { (void)hipFuncSetAttribute((const void*)e.fn, hipFuncAttributeMaxDynamicSharedMemorySize, hp.lds); e.attr = hp.lds; }
    hipLaunchKernelGGL(e.fn, dim3(hp.grid_x, hp.grid_y), dim3(512), hp.lds, stream, p, hp.geo);
    return hipGetLastError();
  }
  return hipErrorInvalidValue;
}

#ifdef DD_TRACE
extern "C" int dd_debug_read_halo_trace(unsigned long long* host, int n) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_halo_trace), sizeof(unsigned long long) * n);
}
#endif
