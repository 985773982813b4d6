// K loop shared by the ping-pong kernels: conv_halo_kernel / conv_halo_persist_kernel (conv_halo.hip) and gemm_pps_kernel (gemm_pps.hip).
// The header of conv_halo.hip says why the loop has this shape; pp_epilogue.h holds what follows it.
#pragma once
#include "common.h"

// LDS row R of a wave's TN * 16 span of a weight stage -> output channel of the tile (which weight row a DMA lane fetches).  Plain form:
// the 16-wide MFMA tiles are paired (2t, 2t + 1) so that a lane's 4 + 4 accumulator rows of a pair are 8 consecutive channels (16-byte
// epilogue stores), exactly as in conv_gemm2.hip; an odd last tile keeps the plain order.  GEGLU (TN = 4, packed (16 hidden | 16 gate)
// groups): a lane holds, per 16-row tile, the hidden AND gate values of 8 consecutive output columns (pp_epilogue_geglu).
template <int TN, bool GEGLU = false>
__device__ __forceinline__ int pp_weight_row(int R) {
  const int wv = R / (TN * 16), q = R - wv * (TN * 16), jn = q >> 4, f = q & 15;
  if (GEGLU) {
    const int c = (f >> 2) * 8 + (jn >> 1) * 4 + (f & 3);          // output column inside the wave's 32
    return wv * 64 + (c >> 4) * 32 + (jn & 1) * 16 + (c & 15);
  }
  return jn < (TN & ~1) ? wv * (TN * 16) + (jn >> 1) * 32 + (f >> 2) * 8 + (jn & 1) * 4 + (f & 3) : R;
}

// One K-step (64 deep) of a wave: two sections, one per 32-deep K half, each a load section (the SIMD partner is in its MFMA section), a
// barrier and 8 x TN MFMAs (the barrier hand-off between the SIMD partners is not hidden by anything: tools/micro/pingpong_gemm.hip,
// four 32-row strips per K-step cost 0.5 us of barrier skeleton per K-step, two K halves 0.35), TN + 8 fragments live instead of 2 TN + 4.
//   Bb               the weight stage (BN rows of 128 B); the wave reads rows wc * TN * 16 ...
//   Xb, x_at(a)      activation fragment a (16 rows) is read from row x_at(a).row of Xb (128 B each).  The 16-byte slots of a row are
//                    swizzled: slot s sits at s ^ key (weights: key = row & 7; x_at(a).key says what the activation rows use)
//   issue_next()     requests of the next K-step, issued in the first half
//   drain            the wait in front of the second half's barrier includes vmcnt(0): this wave's pieces of the next K-step have landed
//                    and its LDS reads of this stage have retired BEFORE the barrier behind which the other half reads the new stage
//                    (false: nothing more of the current tile is in flight, and what is belongs to the next one)
// (x_at gives row and key, not an address: with a callable that returned the pointer hipcc formed every address with one more VALU.)
struct PpRow { int row, key; };
template <int TN, class XAt, class Next>
__device__ __forceinline__ void pp_kstep(f32x4 (&acc)[8][TN], const unsigned char* Bb, const unsigned char* Xb, int wc, int fr, int fq, XAt x_at, Next issue_next,
                                         bool drain) {
  bf16x8 wf[TN], xf[8];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
    for (int jn = 0; jn < TN; ++jn) {
      const int row = wc * (TN * 16) + jn * 16 + fr;
      wf[jn] = *(const bf16x8*)(Bb + row * 128 + (((fq + 4 * ks) ^ (row & 7)) << 4));
    }
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      const PpRow x = x_at(a);
      xf[a] = *(const bf16x8*)(Xb + x.row * 128 + (((fq + 4 * ks) ^ x.key) << 4));
    }
    if (ks == 0) issue_next();
    if (ks == 1) {
      if (drain) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
      for (int jn = 0; jn < TN; ++jn)
        acc[a][jn] = mfma16(wf[jn], xf[a], acc[a][jn]);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_s_barrier();
  }
}

// K loop of one halo tile: chunks [c_begin, c_end) of 64 input channels x the nine taps, which read the SAME staged halo shifted by
// (dy, dx).  At a chunk boundary row group 0 refills the halo (issue_halo(c)) -- every read of the previous chunk's halo has retired: both
// groups waited lgkmcnt(0) in front of their last barrier.  K-step kt of the tile lives in weight stage (kg + kt) & 1 of smem (WB bytes
// each); issue_w(kt) requests this wave's pieces of K-step kt into that stage.  v_taps: lane t holds tap t ((dy + 32) << 6 | (dx + 32)).
// MI: multi-image tiles (+ the two border rows of every 8 x 8 image in front of a pixel's own).
// (narrow form, TN = 1: the second column wave of a row group only multiplies zero padding, columns 16 .. 31.  Letting it skip its
// fragment reads and MFMAs measured SLOWER -- 1206 -> 1504 us on the decoder's conv_out: the form is bound by the exposed halo refill
// of its two short chunks, not by LDS reads, and the branch cost the schedule.)
template <int TN, int WB, bool MI, class IssueHalo, class IssueW>
__device__ __forceinline__ void pp_halo_kloop(f32x4 (&acc)[8][TN], const unsigned char* smem, const unsigned char* halo, int c_begin, int c_end,
                                              int kg, int v_taps, int lw, int grp, int wr, int wc, int fr, int fq, IssueHalo issue_halo,
                                              IssueW issue_w) {
  const int Wd = 1 << lw, W2 = Wd + 2, KT = (c_end - c_begin) * 9;
  int kt = 0;
  for (int c = c_begin; c < c_end; ++c) {
    if (c > c_begin) {
      if (grp == 0) {
        issue_halo(c);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_s_barrier();
    }
    for (int t = 0; t < 9; ++t, ++kt) {
      const int e = __builtin_amdgcn_readlane(v_taps, t);
      const int dy = ((e >> 6) & 63) - 32, dx = (e & 63) - 32;
      const int tapoff = dy * W2 + dx;
      const int st = (kg + kt) & 1;
      const bool more = kt + 1 < KT;
      const int xs = (fr + 1 + dx) & 7;                   // 16-pixel row tiles start at multiples of 16 inside an image row (tw >= 16)
      pp_kstep<TN>(acc, smem + st * WB, halo, wc, fr, fq,
                   [&](int a) {
                     const int r = wr * 128 + a * 16 + fr;
                     return PpRow{r + 2 * (r >> lw) + (MI ? 2 * W2 * (r >> 6) : 0) + Wd + 3 + tapoff, xs};   // halo pixel of output pixel r for this tap
                   },
                   [&] { if (more) issue_w(kt + 1); }, true);
    }
  }
}
