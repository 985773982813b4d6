// K5 / K11 — flash attention forward and backward (dQ, dK, dV) on bf16 MFMA 16x16x32, gfx950.
// Replaces F.scaled_dot_product_attention inside diffusers' Attention processor for UNet self-attention
// (N = 4096/1024/256/64, d = 40/80/160), cross-attention (77 keys; backward needs dQ only) and the VAE
// mid-block single-head attention (d = 512) — reference call sites generate_data.py:112, :701 — and
// its autograd backward (:721, :761).
//
// One design for all three kernels: the "owner" index (queries for fwd/dQ, keys for dK/dV) lives on the
// MFMA column (lane & 15) so every per-row statistic (running max, sum, LSE, delta) is lane-local; the
// streamed side goes through LDS as plain row-major [row][d] tiles (coalesced 16-byte staging) and is
// consumed either by rows (ds_read_b128: QK^T, dO V^T) or by columns (ds_read_b64_tr_b16: P V, dS K, ...).
// Scores are produced transposed (S^T = K Q^T), so the fp32 accumulator registers of S^T are, after
// exp/bf16 packing, directly the B operand of the next MFMA (no LDS round trip, no shuffles): the k-order
// inside a 32-deep step is the permutation key = 32c + 16*(j>>2) + 4*(lane>>4) + (j&3), which is exactly the
// 4-row block order ds_read_b64_tr_b16 delivers. Row stride of the LDS tiles is 2*DPK+32 bytes:
// bank-conflict free for both read kinds (tools/lds_conflicts.py).
// The steps the kernels share (geometry, fragment reads, staging functions, owner rows, score chains, mask, softmax, P.V loop,
// row sum, row epilogue, fp8 P.V) are in attention_frag.h, whose header says which kernel uses which; this file holds the
// kernels' own loops, the planner and the launcher.
#include <cstdlib>
#include <type_traits>
#include "common.h"
#include "kernels.h"
#include "attention_dispatch.h"
#include "attention_frag.h"

namespace {

// ------------------------------------------------------------------------------------------------
// forward.  grid (ceil(Nq / QB), H, B), 256 threads. DSPLIT=1: each wave owns QT 16-query tiles;
// DSPLIT=4: the 4 waves share one set of QT tiles and each accumulates a quarter of the head dim (d=512).
// ------------------------------------------------------------------------------------------------
// Minimum waves per SIMD asked of the register allocator (the second __launch_bounds__ argument), per head dim.  The kernels wait on
// LDS / barriers / exp latency with 2-3 waves per SIMD; one more resident wave is worth more than the few registers it spills
// (tools/bench_attn_occ.py, same device: d = 40 forward 1612 -> 1527 us at 4 waves / 128 VGPRs with 7 spilled registers; d = 80
// 397 -> 327 us at 3 waves / 168 VGPRs, its 77-key cross-attention 91 -> 82 us; NOT for d = 64 at 4 waves (48 spills: 1190 -> 1910 us),
// d = 40 at 5 waves (3x slower) or the backward kernels at 3 waves (d = 40: 1620 -> 1680 us)).
#ifndef DD_AW_FWD
#define DD_AW_FWD(D) ((D) <= 40 ? 4 : (D) <= 80 ? 3 : 1)
#endif
#ifndef DD_AW_DQ
#define DD_AW_DQ(D) 1
#endif
#ifndef DD_AW_DKV
#define DD_AW_DKV(D) 1
#endif
template <int D, int QT, int KT, int DSPLIT, bool CAUSAL>
__global__ __launch_bounds__(256, DD_AW_FWD(D)) void attn_fwd_kernel(AttnParams p) {
  using G = AttnStreamGeo<D, DSPLIT>;
  constexpr int KS = G::KS, DTW = G::DTW, S = G::S, NKT = KT / 16, NC = KT / 32;
  constexpr bool ONES = DSPLIT == 1 && attn_ones(D);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z;
  const int dt0 = G::dt0(wave);

  bf16x8 qf[QT][KS];
  OwnerRow qr[QT];
  f32x4 o[QT][DTW];
  float mrun[QT], lsum[QT];
  int klim[QT];   // first masked key of this lane's query row
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    qr[qt] = owner_row(G::row0(QT, wave) + qt * 16, p.Nq, lane);
    owner_frags<D>(qf[qt], p.q, p.ldq, p.Nq, b, h, qr[qt], lane);
  }
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    klim[qt] = CAUSAL ? min(p.Nk, qr[qt].row + 1) : p.Nk;
    mrun[qt] = -INFINITY; lsum[qt] = 0.f;
#pragma unroll
    for (int dt = 0; dt < DTW; ++dt) o[qt][dt] = splat4(0.f);
  }
  const float sl2 = p.scale * LOG2E;
  const bf16_t* kg = p.k + (size_t)b * p.Nk * p.ldk + h * D;
  const bf16_t* vg = p.v + (size_t)b * p.Nk * p.ldv + h * D;
  unsigned char* Ks = smem;
  unsigned char* Vs = smem + KT * S;
  // K/V tiles are register-staged one tile ahead (global latency hides under the MFMAs of the current tile) for the small
  // head dims; d = 512 keeps the direct staging (its tile would need 64 staging VGPRs)
  constexpr int DPK = G::DPK;
  constexpr bool PREFETCH = (DPK <= 160);
  TileRegs<KT, PREFETCH ? DPK : 32> kreg, vreg;
  if (PREFETCH) {
    tile_load<KT, PREFETCH ? DPK : 32>(kreg, kg, p.ldk, p.Nk, D, tid);
    tile_load<KT, PREFETCH ? DPK : 32, ONES>(vreg, vg, p.ldv, p.Nk, D, tid);
  }
  // the tile body is instantiated twice: PARTIAL (ragged last tile / causal mask) is compile-time, so the full tiles carry none of the
  // mask's compares and index arithmetic (as a run-time test the compiler hoisted them in front of the branch)
  auto tile = [&](auto partial_c, int k0) {
    constexpr bool partial = decltype(partial_c)::value;
    __syncthreads();
    if (PREFETCH) {
      tile_store<KT, PREFETCH ? DPK : 32>(kreg, Ks, S, tid);
      tile_store<KT, PREFETCH ? DPK : 32>(vreg, Vs, S, tid);
    } else {
      stage_tile<KT, DPK>(Ks, S, kg + (size_t)k0 * p.ldk, p.ldk, p.Nk - k0, D, tid);
      stage_tile<KT, DPK, ONES>(Vs, S, vg + (size_t)k0 * p.ldv, p.ldv, p.Nk - k0, D, tid);
    }
    __syncthreads();
    if (PREFETCH && k0 + KT < p.Nk) {
      tile_load<KT, PREFETCH ? DPK : 32>(kreg, kg + (size_t)(k0 + KT) * p.ldk, p.ldk, p.Nk - k0 - KT, D, tid);
      tile_load<KT, PREFETCH ? DPK : 32, ONES>(vreg, vg + (size_t)(k0 + KT) * p.ldv, p.ldv, p.Nk - k0 - KT, D, tid);
    }
    f32x4 st[QT][NKT];
    score_chains(st, Ks, S, qf, lane, [](int, int) { return splat4(0.f); });
    bf16x8 pf[QT][NC];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      if constexpr (partial) mask_keys(st[qt], k0, klim[qt], g);
      online_softmax<ONES>(st[qt], mrun[qt], lsum[qt], o[qt], sl2);
      pack_probs(pf[qt], st[qt]);
    }
    colfrag_mfma(o, Vs, S, pf, dt0, lane);
  };
  {
    int k0 = 0;
    if constexpr (!CAUSAL)
      for (; k0 + KT <= p.Nk; k0 += KT) tile(std::false_type{}, k0);
    for (; k0 < p.Nk; k0 += KT) tile(std::true_type{}, k0);
  }
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const float l = row_sum<D, ONES>(lsum[qt], o[qt][DTW - 1], lane);
    if (!qr[qt].valid()) continue;
    store_row<D>(p.o + ((size_t)b * p.Nq + qr[qt].row) * p.ldo + h * D, o[qt], 1.f / l, dt0, g);
    store_lse(p, b, h, qr[qt].row, mrun[qt], l, g == 0 && (DSPLIT == 1 || wave == 0));
  }
}

// ------------------------------------------------------------------------------------------------
// forward, K/V tiles staged by LDS-DMA (buffer_load_dwordx4 ... lds) into a two-deep ring.  The register-staged form above spends a
// quarter of its time on the staging itself (tools/_attn ablations, DESIGN.md 9.5: global load -> 16 VGPRs -> ds_write_b128, two
// barriers per tile: d = 40 / 4096 keys 1520 us, 1165 us with the staging removed); here a tile is requested one tile ahead with three
// DMA instructions per wave, lands in LDS without touching registers, and one barrier per tile is enough.
// LDS rows are RG 16-byte granules: DG = D / 8 data granules, the rest padding that no DMA lane ever writes (the lanes of the pad
// granules are masked off: an inactive lane leaves its 16-byte slot alone, tools/micro/buflds.hip) -- zeros for K, and for V the
// 1.0 that makes P.V deliver the softmax row sums (ONES).  Row strides (96 B at d <= 40, 160 B at d = 64 / 80) are bank-conflict free for
// the ds_read_b128 row fragments and the ds_read_b64_tr_b16 column fragments (tools/lds_conflicts.py).
// ------------------------------------------------------------------------------------------------
// NW waves per workgroup (4 or 8: eight waves share one K/V ring, half the DMA instructions per query; same waves per SIMD)
// LZ ("lazy reference"): the scores leave the QK^T MFMAs as log2-domain differences to a per-row reference -- Q carries scale * log2(e),
// the first MFMA of every score chain starts from -reference instead of 0 -- so p = exp2(score) needs no fma, and the reference only
// moves when a tile's maximum exceeds it by more than 2^LZ_SLACK (exact in floating point: the reference cancels in O / l; a tile far
// above it is rebased before its exponentials).  The row maximum is still computed, but nothing waits for it.
// FP8 (BASELINE.json configs[4], "fp8 MFMA attention"; AttnParams::pv_fp8, DD_ATTN_FP8=1 in the engine): the P.V product on
// v_mfma_scale_f32_16x16x128_f8f6f4 -- 128 keys per instruction, e4m3 probabilities x e4m3 values, unit block scales, 2x the bf16 rate per
// MAC.  d = 64 only (SDXL's head dim), 128-key tiles.  The probabilities leave the softmax as p = exp2(score - reference) with the
// reference re-based whenever a tile's maximum exceeds it by more than 2^6 (the safe sweep: p <= 64, e4m3 goes to 448), and are packed
// four keys per dword straight from the score accumulators (keys 16 kt + 4 g + r of lane group g: that IS the instruction's 32-byte
// operand).  V is quantised when its tile is staged: the bf16 tile arrives by LDS-DMA as before and the workgroup rewrites it as e4m3 in
// the operand order of the probabilities (row d, lane group g, then (kt, r)), one extra barrier per tile.  QK^T, the softmax, the row
// sums and the LSE stay as they are (bf16 MFMA, fp32).  tools/micro/pv_fp8.hip measured the UPPER bound of the gain on a register-only
// loop: 1.18x; with the in-kernel quantisation pass and 90 KB of LDS (one 8-wave workgroup per CU) this form is not faster than the bf16
// kernel and is not the default.  Accuracy: e4m3 carries 3 mantissa bits (tests/test_kernels_gpu.py states the tolerance).
template <int D, int QT, int KT, int NW, bool LZ, bool FP8 = false>
__global__ __launch_bounds__(NW * 64, FP8 ? 2 : DD_AW_FWD(D)) void attn_fwd_dma_kernel(AttnParams p) {
  static_assert(!FP8 || (D == 64 && KT == 128 && LZ), "fp8 P.V: d = 64, 128-key tiles, lazy-reference softmax");
  using G = AttnLdsGeo<D>;
  constexpr int KS = G::KS, DVT = G::DVT, S = G::RB, RG = G::RG, DG = G::DG;
  constexpr int NKT = KT / 16, NC = KT / 32;
  constexpr int TILE = KT * S;                               // bytes of one K (or V) tile
  constexpr int NPM = KT * RG / 64;                          // DMA pieces (64 granules) per matrix and tile
  constexpr int NPW = (2 * NPM + NW - 1) / NW;               // ... per wave (K pieces first, then V)
  static_assert((KT * RG) % 64 == 0, "tile must be a whole number of 1 KB pieces");
  constexpr bool ONES = attn_ones(D);
  constexpr unsigned OOR = 0xffffff00u;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];    // [buf][K tile | V tile] + 128 B of zeros

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z;

  // ---- padding granules (and the tail behind the last row: the 64-wide K fragments / 16-wide V column tiles read past a row's end)
  for (int r = tid; r < 2 * 2 * KT; r += NW * 64) {              // rows of both buffers, K and V alike
    const bool isv = (r / KT) & 1;
#pragma unroll
    for (int v = DG; v < RG; ++v)
      *(uint4*)(smem + r * S + v * 16) = make_uint4((ONES && isv && v == DG) ? DD_ACT_ONE : 0u, 0, 0, 0);
  }
  if (tid < 8) *(uint4*)(smem + 4 * TILE + tid * 16) = make_uint4(0, 0, 0, 0);
  unsigned char* const VQ = smem + 4 * TILE + 128;          // FP8: the staged V tile as e4m3, [d 64][lane group 4][32 keys] = 8 KB

  bf16x8 qf[QT][KS];
  OwnerRow qr[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    qr[qt] = owner_row((blockIdx.x * NW + wave) * QT * 16 + qt * 16, p.Nq, lane);
    owner_frags<D>(qf[qt], p.q, p.ldq, p.Nq, b, h, qr[qt], lane);
    if (LZ && !p.q_prescaled) {                            // Q not prescaled by the producer: fold scale * log2(e) in here (one more bf16 rounding)
      const float c = p.scale * LOG2E;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        float f[8];
        unpack8(__builtin_bit_cast(uint4, qf[qt][ks]), f);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] *= c;
        qf[qt][ks] = __builtin_bit_cast(bf16x8, pack8(f));
      }
    }
  }
  f32x4 o[QT][DVT];
  float mrun[QT], lsum[QT];
  f32x4 negm[QT];                                           // LZ: -reference of this lane's query row, the start value of its score chains (else 0)
  auto reset = [&] {
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      mrun[qt] = -INFINITY; lsum[qt] = 0.f; negm[qt] = splat4(0.f);
#pragma unroll
      for (int dt = 0; dt < DVT; ++dt) o[qt][dt] = splat4(0.f);
    }
  };
  reset();
  const float sl2 = p.scale * LOG2E;
  const bf16_t* kg = p.k + (size_t)b * p.Nk * p.ldk + h * D;
  const bf16_t* vg = p.v + (size_t)b * p.Nk * p.ldv + h * D;

  // ---- this wave's DMA pieces: piece pc = wave + NW i (pc < NPM: K, else V); lane -> granule pc' * 64 + lane -> (row, granule in row)
  unsigned voff[NPW];
  int prow_[NPW];
#pragma unroll
  for (int i = 0; i < NPW; ++i) {
    const int pc = wave + NW * i, pm = pc < NPM ? pc : pc - NPM;
    const int gi = pm * 64 + lane, row = gi / RG, v = gi - row * RG;
    prow_[i] = v < DG ? row : -1;                            // -1: a padding granule (lane stays off)
    voff[i] = ((unsigned)row * (unsigned)(pc < NPM ? p.ldk : p.ldv) + (unsigned)v * 8u) * 2u;
  }
  auto issue_tile = [&](int k0, int buf) {
    const int nvalid = p.Nk - k0;
#pragma unroll
    for (int i = 0; i < NPW; ++i) {
      const int pc = wave + NW * i;
      if (pc < 2 * NPM) {
        const bool isv = pc >= NPM;
        unsigned char* dst = smem + buf * 2 * TILE + (isv ? TILE : 0) + (isv ? pc - NPM : pc) * 1024;
        if (prow_[i] >= 0)                                   // rows behind the last key are zero-filled by the range check
          dma16(isv ? vg : kg, dst, prow_[i] < nvalid ? voff[i] : OOR, (unsigned)k0 * (unsigned)(isv ? p.ldv : p.ldk) * 2u);
      }
    }
  };
  // One K/V tile.  FIRST / PARTIAL / SAFE are compile-time so that the steady-state instance carries none of the ragged-tile mask
  // arithmetic (the compiler hoisted its 33 compares / index adds in front of the branch when it was a run-time test: a sixth of the
  // vector instructions of a kernel that is bound by the vector issue port) and, for the lazy form, no row maximum at all.
  auto tile = [&](auto first_c, auto partial_c, auto safe_c, int k0, int buf) {
    constexpr bool FIRST = decltype(first_c)::value, PARTIAL = decltype(partial_c)::value, SAFE = decltype(safe_c)::value;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // this wave's pieces of the tile have landed ...
    __syncthreads();                                         // ... everybody's have, and nobody still reads the other buffer
    if (!PARTIAL && k0 + KT < p.Nk) issue_tile(k0 + KT, buf ^ 1);
    const unsigned char* Ks = smem + buf * 2 * TILE;
    const unsigned char* Vs = Ks + TILE;
    // FP8: (everybody finished the previous tile's P.V in front of the barrier above; the barrier in front of this tile's P.V publishes it)
    if constexpr (FP8) fp8_quantise_v<NW * 64>(VQ, Vs, S, tid);
    f32x4 st[QT][NKT];
    score_chains(st, Ks, S, qf, lane, [&](int qt, int) { return LZ ? negm[qt] : splat4(0.f); });
    bf16x8 pf[QT][NC];
    i32x8_t pf8[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      if constexpr (PARTIAL) mask_keys(st[qt], k0, p.Nk, g);  // only the last tile of a ragged key count needs masking
      if constexpr (LZ) {
        // The scores already are differences to the row's reference.  First tile (reference 0: plain scores): the reference becomes
        // the tile's row maximum.  Later tiles: the optimistic pass (SAFE = false) exponentiates them as they are -- no row maximum,
        // nothing to wait for -- and the row sums tell at the end whether a row ran away from its reference (see the tail of the
        // kernel); the safe pass rebases a tile more than 2^LZ_SLACK above the reference before its exponentials (wave-uniform, rare).
#ifdef DD_ACT_F16
        // fp16 probabilities: p <= 2^8 in the safe pass, 2^8 below the largest half (65504).  The optimistic pass has no bound of its
        // own: a p beyond 65504 packs to inf, the P.V MFMA turns it into inf or NaN in every O column (and in the row sum of the ones
        // column), and the finiteness test behind the sweep sends the workgroup to the safe pass.
        constexpr float LZ_SLACK = FP8 ? 6.f : 8.f;
#else
        constexpr float LZ_SLACK = FP8 ? 6.f : 24.f;         // FP8: the probabilities must stay inside e4m3 (448)
#endif
        float mx = 0.f;
        if constexpr (FIRST || SAFE) mx = row_max(st[qt]);
        bool rebase = FIRST;
        if constexpr (!FIRST && SAFE) rebase = __any(mx > LZ_SLACK);
        if (rebase) {
          const float d = FIRST ? mx : fmaxf(mx, 0.f);       // new reference = old + d
          const float alpha = FIRST ? 1.f : __builtin_amdgcn_exp2f(-d);
#pragma unroll
          for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) st[qt][kt][r] -= d;
          if constexpr (!FIRST) {
#pragma unroll
            for (int dt = 0; dt < DVT; ++dt) o[qt][dt] *= alpha;
            if (!ONES) lsum[qt] *= alpha;
          }
          mrun[qt] = (FIRST ? 0.f : mrun[qt]) + d;
          const float nm = -mrun[qt];
          negm[qt] = splat4(nm);
        }
        const float ps = exp2_scores<false, ONES>(st[qt], 1.f, 0.f);
        if (!ONES) lsum[qt] += ps;
      } else {
        online_softmax<ONES>(st[qt], mrun[qt], lsum[qt], o[qt], sl2);
      }
      if constexpr (FP8) pf8[qt] = fp8_pack_probs(st[qt]);
      else pack_probs(pf[qt], st[qt]);
    }
    if constexpr (FP8) {
      __syncthreads();                                       // the e4m3 V tile is complete
      fp8_pv(o, VQ, pf8, lane);
    } else {
      colfrag_mfma(o, Vs, S, pf, 0, lane);
    }
  };
  using T_ = std::true_type;
  using F_ = std::false_type;
  // the whole key loop: tile 0, the full tiles, the ragged last tile
  auto sweep = [&](auto safe_c) {
    issue_tile(0, 0);
    const int nfull = p.Nk / KT;                             // tiles without masking
    if (nfull == 0) { tile(T_{}, T_{}, safe_c, 0, 0); return; }
    tile(T_{}, F_{}, safe_c, 0, 0);
    int buf = 1, k0 = KT;
    for (; k0 < nfull * KT; k0 += KT, buf ^= 1) tile(F_{}, F_{}, safe_c, k0, buf);
    if (k0 < p.Nk) tile(F_{}, T_{}, safe_c, k0, buf);
  };
  if constexpr (LZ) {
    // Optimistic pass: after the first tile no row maximum is taken; p = exp2(score - reference) is exact in bf16 / fp32 whatever its
    // exponent, so the result only depends on the reference through overflow.  A row whose sum left [0, 2^LZ_LIMIT) (or is NaN) ran
    // away from its first tile's maximum by more than any trained attention does; the workgroup then repeats the sweep with the
    // per-tile maximum and the rebase (the decision is workgroup-uniform: the waves share the K/V ring and its barriers).
    constexpr float LZ_LIMIT = 1.8446744e19f;                // 2^64
    bool bad = FP8;                                          // FP8: always the per-tile maximum (the probabilities are bounded by 2^LZ_SLACK)
    if (!FP8) {
      sweep(F_{});
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        const float l = ONES ? o[qt][DVT - 1][(D % 16) % 4] : lsum[qt];     // ONES: only the owning lanes hold the sum, the others hold O columns (bounded by it times |v|)
        bad = bad || !(fabsf(l) < LZ_LIMIT);
#pragma unroll
        for (int dt = 0; dt < DVT; ++dt)
#pragma unroll
          for (int r = 0; r < 4; ++r) bad = bad || !(fabsf(o[qt][dt][r]) < 3.0e38f);
      }
      bad = __syncthreads_or(bad);
    }
    if (bad) { reset(); sweep(T_{}); }
  } else {
    sweep(T_{});
  }
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const float l = row_sum<D, ONES>(lsum[qt], o[qt][DVT - 1], lane);
    if (!qr[qt].valid()) continue;
    store_row<D>(p.o + ((size_t)b * p.Nq + qr[qt].row) * p.ldo + h * D, o[qt], 1.f / l, 0, g);
    store_lse(p, b, h, qr[qt].row, mrun[qt], l, g == 0);
  }
}

// delta[b,h,q] = sum_d dO[q,d] * O[q,d]
__global__ __launch_bounds__(256) void attn_delta_kernel(AttnParams p) {
  const int D = p.D;
  const size_t total = (size_t)p.B * p.H * p.Nq;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    // heads fastest: neighbouring threads read neighbouring D-wide segments of one token row (the rows are [token][head][d])
    const int h = (int)(idx % p.H);
    const int q = (int)((idx / p.H) % p.Nq);
    const int b = (int)(idx / ((size_t)p.Nq * p.H));
    const bf16_t* op = p.o + ((size_t)b * p.Nq + q) * p.ldo + h * D;
    const bf16_t* dp = p.d_o + ((size_t)b * p.Nq + q) * p.lddo + h * D;
    float s = 0.f;
    for (int d = 0; d < D; d += 8) {
      float a[8], c[8];
      unpack8(*(const uint4*)(op + d), a);
      unpack8(*(const uint4*)(dp + d), c);
#pragma unroll
      for (int e = 0; e < 8; ++e) s += a[e] * c[e];
    }
    p.delta[((size_t)b * p.H + h) * p.Nq + q] = s;
  }
}

// ------------------------------------------------------------------------------------------------
// backward dQ: same streaming structure as the forward (keys/values through LDS).
//   dP^T = V dO^T ; dS^T = P^T o (dP^T - delta) ; dQ^T += K^T dS^T
// ------------------------------------------------------------------------------------------------
// PS: the query is prescaled (AttnParams::q_prescaled: scale * log2(e) == 1).  Either way the row constants are the INITIAL accumulators
// of the two score chains -- S starts from -lse (in units of the raw score), dP from -delta -- so p = exp2(S [* scale log2 e]) and dS = p * dP
// need no subtraction per score (cdna_hip_programming.md, attention backward: "Row constants as the initial accumulator").
template <int D, int QT, int KT, int DSPLIT, bool PS>
__global__ __launch_bounds__(256, DD_AW_DQ(D)) void attn_bwd_dq_kernel(AttnParams p) {
  using G = AttnStreamGeo<D, DSPLIT>;
  constexpr int DPK = G::DPK, KS = G::KS, DTW = G::DTW, S = G::S;
  constexpr int NKT = KT / 16, NC = KT / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* Ks = smem;
  unsigned char* Vs = smem + KT * S;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z;
  const int qbase = G::row0(QT, wave), dt0 = G::dt0(wave);

  bf16x8 qf[QT][KS], dof[QT][KS];
  int qrow[QT];
  float lse2[QT], delta[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const OwnerRow orow = owner_row(qbase + qt * 16, p.Nq, lane);
    qrow[qt] = orow.row;
    const bool valid = orow.valid();
    owner_frags<D>(qf[qt], p.q, p.ldq, p.Nq, b, h, orow, lane);
    owner_frags<D>(dof[qt], p.d_o, p.lddo, p.Nq, b, h, orow, lane);
    const size_t si = ((size_t)b * p.H + h) * p.Nq + (valid ? qrow[qt] : 0);
    lse2[qt] = valid ? p.lse[si] * LOG2E : 0.f;
    delta[qt] = valid ? p.delta[si] : 0.f;
  }
  f32x4 dq[QT][DTW];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt)
#pragma unroll
    for (int dt = 0; dt < DTW; ++dt) dq[qt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float sl2 = p.scale * LOG2E;
  const bf16_t* kg = p.k + (size_t)b * p.Nk * p.ldk + h * D;
  const bf16_t* vg = p.v + (size_t)b * p.Nk * p.ldv + h * D;

  // initial accumulators of the score chains (per query row = per lane: the row sits on the MFMA column)
  f32x4 sinit[QT], dinit[QT];
  {
    const float isl2 = PS ? 1.f : 1.f / sl2;
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      const float a = -lse2[qt] * isl2, d = -delta[qt];
      sinit[qt] = f32x4{a, a, a, a};
      dinit[qt] = f32x4{d, d, d, d};
    }
  }
  // K/V tiles are register-staged one tile ahead like the forward (the global latency hides under the previous tile's MFMAs)
  constexpr bool PREFETCH = (DPK <= 160);
  TileRegs<KT, PREFETCH ? DPK : 32> kreg, vreg;
  if (PREFETCH) {
    tile_load<KT, PREFETCH ? DPK : 32>(kreg, kg, p.ldk, p.Nk, D, tid);
    tile_load<KT, PREFETCH ? DPK : 32>(vreg, vg, p.ldv, p.Nk, D, tid);
  }
  // RAGGED (keys beyond Nk: only the last tile of a ragged key count) is compile-time: as a run-time test the compiler kept the 64
  // selects and their compares in every tile
  auto tile = [&](auto ragged_c, int k0) {
    constexpr bool ragged = decltype(ragged_c)::value;
    __syncthreads();
    if (PREFETCH) {
      tile_store<KT, PREFETCH ? DPK : 32>(kreg, Ks, S, tid);
      tile_store<KT, PREFETCH ? DPK : 32>(vreg, Vs, S, tid);
    } else {
      stage_tile<KT, DPK>(Ks, S, kg + (size_t)k0 * p.ldk, p.ldk, p.Nk - k0, D, tid);
      stage_tile<KT, DPK>(Vs, S, vg + (size_t)k0 * p.ldv, p.ldv, p.Nk - k0, D, tid);
    }
    __syncthreads();
    if (PREFETCH && k0 + KT < p.Nk) {
      tile_load<KT, PREFETCH ? DPK : 32>(kreg, kg + (size_t)(k0 + KT) * p.ldk, p.ldk, p.Nk - k0 - KT, D, tid);
      tile_load<KT, PREFETCH ? DPK : 32>(vreg, vg + (size_t)(k0 + KT) * p.ldv, p.ldv, p.Nk - k0 - KT, D, tid);
    }
    bf16x8 dsf[QT][NC];
    {
      f32x4 st[QT][NKT], dpt[QT][NKT];
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) { st[qt][kt] = sinit[qt]; dpt[qt][kt] = dinit[qt]; }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const bf16x8 kf = lds_row_frag(Ks, kt * 16 + i16, S, g + 4 * ks);
          const bf16x8 vf = lds_row_frag(Vs, kt * 16 + i16, S, g + 4 * ks);
#pragma unroll
          for (int qt = 0; qt < QT; ++qt) {
            st[qt][kt] = mfma16(kf, qf[qt][ks], st[qt][kt]);
            dpt[qt][kt] = mfma16(vf, dof[qt][ks], dpt[qt][kt]);
          }
        }
      }
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float pr = __builtin_amdgcn_exp2f(PS ? st[qt][kt][r] : st[qt][kt][r] * sl2);
            if constexpr (ragged) { if (k0 + kt * 16 + 4 * g + r >= p.Nk) pr = 0.f; }
            st[qt][kt][r] = pr * dpt[qt][kt][r];
          }
#pragma unroll
        for (int c = 0; c < NC; ++c) dsf[qt][c] = pack_frag(st[qt][2 * c], st[qt][2 * c + 1]);
      }
    }
#pragma unroll
    for (int dt = 0; dt < DTW; ++dt)
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const bf16x8 kcf = lds_col_frag(Ks, 32 * c, S, dt0 + dt, lane);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) dq[qt][dt] = mfma16(kcf, dsf[qt][c], dq[qt][dt]);
      }
  };
  {
    int k0 = 0;
    for (; k0 + KT <= p.Nk; k0 += KT) tile(std::false_type{}, k0);
    if (k0 < p.Nk) tile(std::true_type{}, k0);
  }
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    if (qrow[qt] >= p.Nq) continue;
    bf16_t* op = p.dq + ((size_t)b * p.Nq + qrow[qt]) * p.lddq + h * D;
    store_row<D>(op, dq[qt], p.scale, dt0, g);
  }
}

// ------------------------------------------------------------------------------------------------
// backward dK/dV: keys own the lanes, queries (Q, dO, LSE, delta) stream through LDS.
//   S = Q K^T ; P = exp(S*scale - LSE) ; dP = dO V^T ; dS = P o (dP - delta)
//   dV^T += dO^T P ; dK^T += Q^T dS
// ------------------------------------------------------------------------------------------------
template <int D, int KTW, int QTL, int DSPLIT, bool PS>
__global__ __launch_bounds__(256, DD_AW_DKV(D)) void attn_bwd_dkv_kernel(AttnParams p) {
  using G = AttnStreamGeo<D, DSPLIT>;
  constexpr int DPK = G::DPK, KS = G::KS, DTW = G::DTW, S = G::S;
  constexpr int NQT = QTL / 16, NC = QTL / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* Qs = smem;
  unsigned char* Os = smem + QTL * S;
  float* ls = (float*)(smem + 2 * QTL * S);   // [QTL] -lse (in raw-score units), then [QTL] -delta: the initial accumulators of S and dP

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z;
  const int kbase = G::row0(KTW, wave), dt0 = G::dt0(wave);

  bf16x8 kf[KTW][KS], vf[KTW][KS];
  int krow[KTW];
#pragma unroll
  for (int kt = 0; kt < KTW; ++kt) {
    const OwnerRow orow = owner_row(kbase + kt * 16, p.Nk, lane);
    krow[kt] = orow.row;
    owner_frags<D>(kf[kt], p.k, p.ldk, p.Nk, b, h, orow, lane);
    owner_frags<D>(vf[kt], p.v, p.ldv, p.Nk, b, h, orow, lane);
  }
  f32x4 dk[KTW][DTW], dv[KTW][DTW];
#pragma unroll
  for (int kt = 0; kt < KTW; ++kt)
#pragma unroll
    for (int dt = 0; dt < DTW; ++dt) { dk[kt][dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[kt][dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  const float sl2 = p.scale * LOG2E;
  const bf16_t* qg = p.q + (size_t)b * p.Nq * p.ldq + h * D;
  const bf16_t* og = p.d_o + (size_t)b * p.Nq * p.lddo + h * D;
  const float* lseg = p.lse + ((size_t)b * p.H + h) * p.Nq;
  const float* delg = p.delta + ((size_t)b * p.H + h) * p.Nq;

  // Q / dO tiles (and their lse / delta rows) are register-staged one tile ahead for the small head dims
  constexpr bool PREFETCH = (DPK <= 160);
  TileRegs<QTL, PREFETCH ? DPK : 32> qreg, oreg;
  float lreg = -INFINITY, dreg = 0.f;
  auto load_rows = [&](int q0) {
    if (tid < QTL) {
      const bool v = q0 + tid < p.Nq;
      lreg = v ? -lseg[q0 + tid] * (PS ? LOG2E : LOG2E / sl2) : -INFINITY;      // -inf -> P = 0 for padded query rows
      dreg = v ? -delg[q0 + tid] : 0.f;
    }
  };
  if (PREFETCH) {
    tile_load<QTL, PREFETCH ? DPK : 32>(qreg, qg, p.ldq, p.Nq, D, tid);
    tile_load<QTL, PREFETCH ? DPK : 32>(oreg, og, p.lddo, p.Nq, D, tid);
    load_rows(0);
  }
  for (int q0 = 0; q0 < p.Nq; q0 += QTL) {
    __syncthreads();
    if (PREFETCH) {
      tile_store<QTL, PREFETCH ? DPK : 32>(qreg, Qs, S, tid);
      tile_store<QTL, PREFETCH ? DPK : 32>(oreg, Os, S, tid);
    } else {
      stage_tile<QTL, DPK>(Qs, S, qg + (size_t)q0 * p.ldq, p.ldq, p.Nq - q0, D, tid);
      stage_tile<QTL, DPK>(Os, S, og + (size_t)q0 * p.lddo, p.lddo, p.Nq - q0, D, tid);
      load_rows(q0);
    }
    if (tid < QTL) { ls[tid] = lreg; ls[QTL + tid] = dreg; }
    __syncthreads();
    if (PREFETCH && q0 + QTL < p.Nq) {
      tile_load<QTL, PREFETCH ? DPK : 32>(qreg, qg + (size_t)(q0 + QTL) * p.ldq, p.ldq, p.Nq - q0 - QTL, D, tid);
      tile_load<QTL, PREFETCH ? DPK : 32>(oreg, og + (size_t)(q0 + QTL) * p.lddo, p.lddo, p.Nq - q0 - QTL, D, tid);
      load_rows(q0 + QTL);
    }
    bf16x8 pf[KTW][NC], dsf[KTW][NC];
    {
      f32x4 s[KTW][NQT], dp[KTW][NQT];
#pragma unroll
      for (int qt = 0; qt < NQT; ++qt) {
        // the first K slice accumulates onto the row constants of its four query rows: -lse for S, -delta for dP
        const f32x4 sin4 = *(const f32x4*)(ls + qt * 16 + 4 * g), din4 = *(const f32x4*)(ls + QTL + qt * 16 + 4 * g);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const bf16x8 qfr = lds_row_frag(Qs, qt * 16 + i16, S, g + 4 * ks);
          const bf16x8 ofr = lds_row_frag(Os, qt * 16 + i16, S, g + 4 * ks);
#pragma unroll
          for (int kt = 0; kt < KTW; ++kt) {
            s[kt][qt] = mfma16(qfr, kf[kt][ks], ks == 0 ? sin4 : s[kt][qt]);
            dp[kt][qt] = mfma16(ofr, vf[kt][ks], ks == 0 ? din4 : dp[kt][qt]);
          }
        }
      }
      // s[kt][qt][r] = S[q = q0 + qt*16 + 4g + r][key = krow[kt]]
#pragma unroll
      for (int qt = 0; qt < NQT; ++qt) {
#pragma unroll
        for (int kt = 0; kt < KTW; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float pr = __builtin_amdgcn_exp2f(PS ? s[kt][qt][r] : s[kt][qt][r] * sl2);
            s[kt][qt][r] = pr;
            dp[kt][qt][r] = pr * dp[kt][qt][r];
          }
      }
#pragma unroll
      for (int kt = 0; kt < KTW; ++kt)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          pf[kt][c] = pack_frag(s[kt][2 * c], s[kt][2 * c + 1]);
          dsf[kt][c] = pack_frag(dp[kt][2 * c], dp[kt][2 * c + 1]);
        }
    }
#pragma unroll
    for (int dt = 0; dt < DTW; ++dt)
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const bf16x8 ocf = lds_col_frag(Os, 32 * c, S, dt0 + dt, lane);
        const bf16x8 qcf = lds_col_frag(Qs, 32 * c, S, dt0 + dt, lane);
#pragma unroll
        for (int kt = 0; kt < KTW; ++kt) {
          dv[kt][dt] = mfma16(ocf, pf[kt][c], dv[kt][dt]);
          dk[kt][dt] = mfma16(qcf, dsf[kt][c], dk[kt][dt]);
        }
      }
  }
#pragma unroll
  for (int kt = 0; kt < KTW; ++kt) {
    if (krow[kt] >= p.Nk) continue;
    bf16_t* kp = p.dk + ((size_t)b * p.Nk + krow[kt]) * p.lddk + h * D;
    bf16_t* vp = p.dv + ((size_t)b * p.Nk + krow[kt]) * p.lddv + h * D;
    store_row<D>(kp, dk[kt], p.scale, dt0, g);
    store_row<D>(vp, dv[kt], 1.f, dt0, g);
  }
}


// ------------------------------------------------------------------------------------------------
// host side: the kernels of one plan.  The causal mask (CLIP text encoder, forward only) and the prescaled query are template flags:
// the UNet / VAE loops carry no per-score mask code
// ------------------------------------------------------------------------------------------------
template <int I>
hipError_t launch_fwd_form(const AttnParams& p, const AttnPlan& plan, hipStream_t s) {
  constexpr AttnForm F = ATTN_FORMS[I];
  const AttnLaunch& l = plan.launch[0];
  if (plan.route == ATTN_DMA) {
    if constexpr (F.fp8) return launch_dyn_lds<attn_fwd_dma_kernel<F.d, F.qt, F.kt, 8, true, true>>(l.grid, l.block, l.lds, s, p);
    else if constexpr (F.dma()) {
      if constexpr (F.dma8()) {
        if (plan.waves == 8)
          return plan.lazy ? launch_dyn_lds<attn_fwd_dma_kernel<F.d, F.qt, F.kt, 8, true>>(l.grid, l.block, l.lds, s, p)
                           : launch_dyn_lds<attn_fwd_dma_kernel<F.d, F.qt, F.kt, 8, false>>(l.grid, l.block, l.lds, s, p);
      }
      return plan.lazy ? launch_dyn_lds<attn_fwd_dma_kernel<F.d, F.qt, F.kt, 4, true>>(l.grid, l.block, l.lds, s, p)
                       : launch_dyn_lds<attn_fwd_dma_kernel<F.d, F.qt, F.kt, 4, false>>(l.grid, l.block, l.lds, s, p);
    }
    return hipErrorInvalidValue;
  }
  if constexpr (!F.fp8)
    return plan.causal ? launch_dyn_lds<attn_fwd_kernel<F.d, F.qt, F.kt, F.dsplit, true>>(l.grid, l.block, l.lds, s, p)
                       : launch_dyn_lds<attn_fwd_kernel<F.d, F.qt, F.kt, F.dsplit, false>>(l.grid, l.block, l.lds, s, p);
  return hipErrorInvalidValue;
}
template <int I>
hipError_t launch_bwd_form(const AttnParams& p, const AttnPlan& plan, hipStream_t s) {
  constexpr AttnForm F = ATTN_FORMS[I];
  if constexpr (F.dq_qt > 0) {
    const AttnLaunch& q = plan.launch[1];
    const hipError_t e = plan.prescaled ? launch_dyn_lds<attn_bwd_dq_kernel<F.d, F.dq_qt, F.dq_kt, F.dsplit, true>>(q.grid, q.block, q.lds, s, p)
                                        : launch_dyn_lds<attn_bwd_dq_kernel<F.d, F.dq_qt, F.dq_kt, F.dsplit, false>>(q.grid, q.block, q.lds, s, p);
    if (e != hipSuccess || plan.launches < 3) return e;
    const AttnLaunch& k = plan.launch[2];
    return plan.prescaled ? launch_dyn_lds<attn_bwd_dkv_kernel<F.d, F.ktw, F.qtl, F.dsplit, true>>(k.grid, k.block, k.lds, s, p)
                          : launch_dyn_lds<attn_bwd_dkv_kernel<F.d, F.ktw, F.qtl, F.dsplit, false>>(k.grid, k.block, k.lds, s, p);
  }
  return hipErrorInvalidValue;
}

AttnLaunch delta_launch(const AttnParams& p) {
  const size_t total = (size_t)p.B * p.H * p.Nq;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  return AttnLaunch{dim3(blocks), 256, 0};
}

hipError_t run_plan(const AttnParams& p, const AttnScratch& scratch, const AttnPlan& plan, bool bwd, hipStream_t s) {
  switch (plan.route) {
    case ATTN_GEMM:
      if (bwd) { const hipError_t e = launch_attention_delta(p, s); if (e != hipSuccess) return e; }
      return launch_attention_gemm(p, scratch, plan.group, bwd, s);
    case ATTN_SHORTK: return launch_attention_shortk(p, plan, s);
    case ATTN_DMA:
    case ATTN_STREAM: return attn_with_form(plan.form, [&](auto i) { return launch_fwd_form<decltype(i)::value>(p, plan, s); });
    case ATTN_FLASH_BWD: {
      const hipError_t e = launch_attention_delta(p, s);
      if (e != hipSuccess) return e;
      return attn_with_form(plan.form, [&](auto i) { return launch_bwd_form<decltype(i)::value>(p, plan, s); });
    }
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

// The only place that decides refusal, route and form.  Order: the GEMM route if scratch is offered, the shape is its own and (backward)
// dk / dv are asked for; then the short-key kernel; fp8 P.V; the LDS-DMA staged kernel on 8 or 4 waves; the register-staged kernel.
AttnPlan attention_plan(const AttnParams& p, const AttnScratch& sc, bool bwd, int force) {
  AttnPlan plan;
  if (p.Nq <= 0 || p.Nk <= 0) return plan;
#ifdef DD_ACT_F16
  if (p.pv_fp8) return plan;                                   // the fp16 build has no fp8 P.V form (its V quantisation pass reads bf16 tiles)
#endif
  const bool ld8 = !(p.ldq & 7) && !(p.ldk & 7) && !(p.ldv & 7);
  if (sc.workspace && sc.tap1x1 && attn_gemm_shape(p.Nq, p.Nk, p.D, p.causal) && ld8 && !(p.ldo & 7) && (!bwd || (p.dk && p.dv)) &&
      sc.workspace_bytes >= attention_gemm_workspace(p.Nq, p.Nk, p.D, bwd)) {
    if (!p.lse) return plan;
    if (bwd && (!p.delta || !p.d_o || !p.o || !p.dq || (p.lddo & 7) || (p.lddq & 7) || (p.lddk & 7) || (p.lddv & 7))) return plan;
    plan.route = ATTN_GEMM;
    const size_t fit = sc.workspace_bytes / attention_gemm_workspace(p.Nq, p.Nk, p.D, bwd);
    const int gmax = attn_gemm_group_max(p.B, p.H, p.Nq, p.Nk);
    plan.group = fit < (size_t)gmax ? (int)fit : gmax;
    return plan;
  }
  if (force == ATTN_GEMM || !ld8 || (p.ldo & 3)) return plan;
  const int form = attn_form_of(p.D);
  const auto grid = [&](int rows, int per) { return dim3((rows + per - 1) / per, p.H, p.B); };
  if (bwd) {
    if ((p.lddo & 7) || (p.lddq & 3) || !p.delta || !p.lse || !p.d_o || !p.o || form < 0) return plan;
    if (p.dk && ((p.lddk & 3) || (p.lddv & 3))) return plan;
    const AttnForm& f = ATTN_FORMS[form];
    const int span = attn_stream_span(f.dsplit), S = attn_stream_row_bytes(f.d);    // rows of a 16-row tile over the workgroup, LDS row bytes
    plan.route = ATTN_FLASH_BWD; plan.form = form; plan.waves = 4; plan.prescaled = p.q_prescaled != 0;
    plan.launch[0] = delta_launch(p);
    plan.launch[1] = AttnLaunch{grid(p.Nq, span * f.dq_qt), 256, (size_t)2 * f.dq_kt * S};
    plan.launch[2] = AttnLaunch{grid(p.Nk, span * f.ktw), 256, (size_t)2 * f.qtl * S + 2 * f.qtl * sizeof(float)};
    plan.launches = p.dk ? 3 : 2;
    return plan;
  }
  const bool kv_fit = offsets_fit_32bit(p.Nk, p.ldk > p.ldv ? p.ldk : p.ldv);
  // short keys: non-causal, <= 80 keys, whole 32-query tiles, a head dim with a short-key kernel, rows within the 32-bit byte offsets of one image
  if (form >= 0 && ATTN_FORMS[form].sk_nw && attn_env().shortk && !p.no_shortk && !p.causal && !p.pv_fp8 && p.Nk <= 80 && !(p.Nq & 31) &&
      offsets_fit_32bit(p.Nq, p.ldq) && kv_fit) {
    const int nw = ATTN_FORMS[form].sk_nw, rb = attn_dma_row_bytes(p.D);
    const int qslot = (32 * rb + 1023) / 1024 * 1024, npk = (96 * rb + 1023) / 1024;   // bytes of a wave's Q slot, 1 KB pieces of the K (or V) block
    plan.route = ATTN_SHORTK; plan.form = form; plan.waves = nw;
    plan.sk_tiles = p.Nq / 32;
    // tiles per wave: enough workgroups to fill the chip twice over, at most 8 tiles per wave (the K / V staging is amortised over them)
    int wgs = (plan.sk_tiles + nw - 1) / nw;                   // one tile per wave
    int per = 8;
    while (per > 1 && (long long)((wgs + per - 1) / per) * p.H * p.B < 1024) per >>= 1;
    plan.sk_wgs = (wgs + per - 1) / per;
    plan.launch[0] = AttnLaunch{dim3(((p.B * plan.sk_wgs + 7) & ~7) * p.H), (unsigned)nw * 64, (size_t)2 * npk * 1024 + (size_t)nw * 2 * qslot};
    plan.launches = 1;
    return plan;
  }
  if (form < 0) return plan;
  // fp8 P.V (BASELINE.json configs[4]): opt-in per launch, d = 64, non-causal, key / value rows within the LDS-DMA offset range
  const bool fp8 = p.pv_fp8 && p.D == ATTN_FORMS[ATTN_FORM_FP8].d && !p.causal && kv_fit;
  const AttnForm& f = ATTN_FORMS[fp8 ? ATTN_FORM_FP8 : form];
  plan.form = fp8 ? ATTN_FORM_FP8 : form;
  plan.launches = 1;
  if (fp8 || (f.dma() && !p.causal && kv_fit)) {
    plan.route = ATTN_DMA; plan.fp8 = fp8; plan.lazy = fp8 || p.q_prescaled;
    plan.waves = fp8 || (f.dma8() && p.Nq % (8 * f.qt * 16) == 0) ? 8 : 4;
    plan.launch[0] = AttnLaunch{grid(p.Nq, plan.waves * f.qt * 16), (unsigned)plan.waves * 64, (size_t)4 * f.kt * attn_dma_row_bytes(f.d) + 128 + (fp8 ? 8192 : 0)};
    return plan;
  }
  plan.route = ATTN_STREAM; plan.waves = 4; plan.causal = p.causal != 0;
  plan.launch[0] = AttnLaunch{grid(p.Nq, attn_stream_span(f.dsplit) * f.qt), 256, (size_t)2 * f.kt * attn_stream_row_bytes(f.d)};
  return plan;
}

int attention_plan_query(const AttnParams& p, size_t workspace_bytes, bool bwd, int* out) {
  static int some_scratch;                                     // the planner tests the scratch pointers for null and never follows them
  const AttnScratch sc = workspace_bytes ? AttnScratch{&some_scratch, workspace_bytes, &some_scratch, nullptr, 0} : AttnScratch{};
  const AttnPlan plan = attention_plan(p, sc, bwd);
  for (int i = 0; i < 26; ++i) out[i] = 0;
  out[0] = plan.route;
  if (plan.route < 0) return plan.route;
  if (plan.route == ATTN_GEMM) { out[9] = plan.group; return plan.route; }
  const AttnForm& f = ATTN_FORMS[plan.form];
  out[1] = f.d; out[4] = plan.route == ATTN_SHORTK ? 0 : f.dsplit;
  if (bwd) { out[2] = f.dq_qt; out[3] = f.dq_kt; if (plan.launches == 3) { out[5] = f.ktw; out[6] = f.qtl; } }
  else if (plan.route != ATTN_SHORTK) { out[2] = f.qt; out[3] = f.kt; }
  out[7] = plan.waves;
  out[8] = (plan.lazy ? 1 : 0) | (plan.prescaled ? 2 : 0) | (plan.causal ? 4 : 0) | (plan.fp8 ? 8 : 0);
  out[10] = plan.launches;
  for (int i = 0; i < plan.launches; ++i) {
    const AttnLaunch& l = plan.launch[i];
    out[11 + 5 * i] = (int)l.grid.x; out[12 + 5 * i] = (int)l.grid.y; out[13 + 5 * i] = (int)l.grid.z; out[14 + 5 * i] = (int)l.block; out[15 + 5 * i] = (int)l.lds;
  }
  return plan.route;
}

size_t attention_scratch_bytes(int B, int heads, int Nq, int Nk, int D, bool causal, bool cross, bool want_grad) {
  if (cross || !attn_gemm_shape(Nq, Nk, D, causal)) return 0;
  return attention_gemm_workspace(Nq, Nk, D, want_grad ? 1 : 0) * (size_t)attn_gemm_group_max(B, heads, Nq, Nk);
}

hipError_t launch_attention(const AttnParams& p, const AttnScratch& scratch, bool bwd, hipStream_t s) {
  return run_plan(p, scratch, attention_plan(p, scratch, bwd), bwd, s);
}
hipError_t launch_attention_fwd(const AttnParams& p, hipStream_t s) { return launch_attention(p, AttnScratch{}, false, s); }
hipError_t launch_attention_bwd(const AttnParams& p, hipStream_t s) { return launch_attention(p, AttnScratch{}, true, s); }
hipError_t launch_attention_gemm_fwd(const AttnParams& p, void* workspace, size_t workspace_bytes, const int* tap1x1, float* partial, size_t partial_cap, hipStream_t s) {
  const AttnScratch sc{workspace, workspace_bytes, tap1x1, partial, partial_cap};
  return run_plan(p, sc, attention_plan(p, sc, false, ATTN_GEMM), false, s);
}
hipError_t launch_attention_gemm_bwd(const AttnParams& p, void* workspace, size_t workspace_bytes, const int* tap1x1, float* partial, size_t partial_cap, hipStream_t s) {
  const AttnScratch sc{workspace, workspace_bytes, tap1x1, partial, partial_cap};
  return run_plan(p, sc, attention_plan(p, sc, true, ATTN_GEMM), true, s);
}

hipError_t launch_attention_delta(const AttnParams& p, hipStream_t s) {
  if (!p.delta || !p.d_o || !p.o) return hipErrorInvalidValue;
  const AttnLaunch l = delta_launch(p);
  hipLaunchKernelGGL(attn_delta_kernel, l.grid, dim3(l.block), 0, s, p);
  return hipGetLastError();
}
