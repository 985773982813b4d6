// Host-side launch interface of the hand-written gfx950 kernels.
// Everything here enqueues on the given stream and never synchronises.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef unsigned short bf16_t;

// ----------------------------------------------------------------------------------------------
// K1/K2/K8: implicit-GEMM convolution == GEMM == linear (bf16 MFMA, fp32 accumulate).
//   out[m, n] = epilogue( alpha * sum_k A[m, k] * Wp[n, k] ),  m = (b, oy, ox) NHWC pixel,
//   k = (tap, cin) with cin fastest, A gathered on the fly from the NHWC input (zero padding,
//   optional fused nearest-2x upsample, optional stride-2, optional input-dilated "transposed"
//   gather used for the dgrad of stride-2 convolutions).
// ----------------------------------------------------------------------------------------------
enum ConvFlags {
  CF_BIAS = 1,       // + bias[n]          (fp32; optionally selected per timestep through bias_sel)
  CF_RES = 2,        // + res[m, n]        (bf16)
  CF_RELU = 4,       // max(., 0)
  CF_GEGLU = 8,      // packed (hidden|gate) 16-column groups -> hidden * gelu(gate); N counts packed columns
  CF_OUT_F32 = 16,   // store fp32 instead of bf16
  CF_MASK = 32,      // multiply by (mask[m, n] > 0)   (ReLU backward)
  CF_RES_F32 = 64,   // residual is fp32
  CF_GEGLU_RAW = 128,// with CF_GEGLU: also store the raw packed pre-activation (bf16) to raw[m, N]
  CF_RELU6 = 512,    // min(max(., 0), 6)   (fp32 guide kernels: MobileNetV2)
  CF_STATS = 256,    // also emit per-(64-row block, output channel) partial statistics (mean, M2) of the stored values: the
                     // GroupNorm that consumes this tensor then needs no statistics pass of its own (conv_gemm_can_emit_stats)
  CF_LNFOLD = 1024,  // the A operand is the RAW input x of a LayerNorm whose gamma is folded into the packed weights (W' = gamma o W) and
                     // whose beta into the bias (b' = b + W beta): out = alpha * rstd[m] * (acc - mean[m] * c1[n]) + b'[n] with
                     // c1[n] = sum_k W'[n, k] (of the bf16-rounded W'), (mean, rstd) = ln_stats[m] -- LayerNorm(x) W^T + b without ever
                     // materialising LayerNorm(x).  Pointwise (1x1 / linear) layers only.
  CF_ROWSTATS = 2048 // also emit, per output row and per 80-/64-column wave span, (sum v, sum v^2) of the fp32 values in front of their bf16 rounding
                     // (one-pass fp32: rstd of the stored rows within 4 % up to |mean| = 50 std, tests/test_kernels_gpu.py) into rowpart: the
                     // LayerNorm that consumes this tensor takes its row statistics from there (conv_gemm_can_emit_rowstats)
};

struct ConvGemmParams {
  const bf16_t* x;      // input activations, NHWC, row stride x_ld elements
  const bf16_t* w;      // packed weights [N][K], K contiguous, K % 64 == 0 (zero padded)
  const int* taptab;    // ntaps entries: ((dy + 32) << 6) | (dx + 32), logical-input offset of each filter tap
  void* y;              // output (bf16 or fp32), row stride y_ld
  const float* bias;    // [N] fp32 or null
  const int* bias_sel;  // optional device scalar: bias += (*bias_sel) * bias_stride
  const void* res;      // residual or null
  const bf16_t* mask;   // relu mask source or null
  bf16_t* raw;          // GEGLU raw output or null
  float* partial;       // split-K workspace [ksplit][M][N] fp32 (ksplit > 1)
  float* stats;         // CF_STATS: [M / 64][stats_ld][2] fp32 (mean, M2 of 64 rows), already offset to this op's first channel
  const float* ln_stats;// CF_LNFOLD: [M][2] fp32 (mean, rstd) of the LayerNorm's input rows
  const float* ln_c1;   // CF_LNFOLD: [N] fp32 column sums of the folded weights (packed order for GEGLU)
  float* rowpart;       // CF_ROWSTATS: [M][rowpart_ld][2] fp32 (sum, sum of squares) per row and column span of conv_gemm_rowstat_span(N)
  int x_ld, y_ld, res_ld, mask_ld, raw_ld, bias_stride, stats_ld, rowpart_ld;
  int B, H, W;          // stored input geometry
  int Ho, Wo;           // output geometry
  int stride;           // output->logical-input stride (1 or 2)
  int shift;            // 1: logical input is 2x the stored input (nearest upsample or dilation)
  int parity;           // 1 with shift: only even logical coordinates are populated (transposed conv)
  int cin, ntaps;       // channels per tap (multiple of 8), number of taps; K = roundup(ntaps*cin, 64)
  int M, N, K;
  int ksplit;
  int flags;
  float alpha;
  int force_small;      // diagnostics: 1 forces the 128x128-tile kernel
  int wgroup_rows;      // > 0: GROUPED weights -- output rows [g * wgroup_rows, (g + 1) * wgroup_rows) use the weight matrix at
  long long wgroup_elems; //   w + g * wgroup_elems (same [N][K] shape each): a batch of independent GEMMs stacked along M in one launch
                        //   (attention_gemm.hip: S_b = Q_b K_b^T for all images b).  Persistent big-tile kernel only; 0 otherwise.
};

// Chooses tile configuration / split-K from the shape. `partial_cap_bytes` bounds split-K workspace.
hipError_t launch_conv_gemm(ConvGemmParams p, size_t partial_cap_bytes, hipStream_t stream);
// The kernel launch_conv_gemm(p, partial_cap_bytes) would run (the launcher's own decision code, nothing is launched): 0 the general
// kernels (conv_gemm_kernel / conv_gemm_big_kernel), 1 conv_halo_kernel, 2 conv_halo_persist_kernel, 3 gemm_ws_kernel, 4 gemm_pps_kernel;
// -1 when the launcher would refuse the problem
int conv_gemm_kind(ConvGemmParams p, size_t partial_cap_bytes);
// The same decision with the form inside the kind: returns the kind and fills out4 = {kind, conv_gemm_big_kernel configuration (0: the
// small conv_gemm_kernel; 1 128 x 256, 2 256 x 160, 3 256 x 128 on 8 waves; 4 128 x 160, 5 128 x 128 as two 4-wave workgroups per CU),
// the split-K (8 x 8 halo level: chunk split) the launch uses, 1 when the small kernel runs 256 x 64 tiles instead of 128 x 128}
int conv_gemm_plan_query(ConvGemmParams p, size_t partial_cap_bytes, int* out4);
// What the launch does beyond the bits when a halo kernel runs the problem: 0 when none would, else 1 and out12 = {kind, HALO_FORMS id,
// tile width, tile height, tiles per image row, tile rows per image, images per tile, halo address table 0 / 1, dynamic LDS bytes, grid x,
// grid y (the chunk split), persistent 0 / 1}
int conv_halo_plan_query(ConvGemmParams p, size_t partial_cap_bytes, int* out12);
// Preferred split for a shape (used by the engine to size the workspace).
int conv_gemm_pick_split(int M, int N, int K);
// true iff launch_conv_gemm(p, partial_cap_bytes) will honour CF_STATS for this problem (persistent big-tile kernel, no split-K,
// M % 64 == 0, plain bf16 output): the caller asks before setting the flag and falls back to the GroupNorm statistics pass otherwise
bool conv_gemm_can_emit_stats(ConvGemmParams p, size_t partial_cap_bytes);
// CF_ROWSTATS: true iff launch_conv_gemm will honour it for this problem; *spans = number of (sum, sum^2) pairs per row it writes
// (N / columns per wave of the tile the launcher picks); rowpart_ld must be >= *spans
bool conv_gemm_can_emit_rowstats(ConvGemmParams p, size_t partial_cap_bytes, int* spans);

// ----------------------------------------------------------------------------------------------
// K3: GroupNorm (+ optional SiLU) forward / backward on NHWC bf16.
// ----------------------------------------------------------------------------------------------
struct GroupNormParams {
  const bf16_t* x; int x_ld;
  bf16_t* y; int y_ld;
  const float* gamma; const float* beta;   // [C]
  float* stats;        // [B][G][2] (mean, rstd), written by fwd, read by bwd
  float* scratch;      // [B][S][G][3] partial (count, mean, M2) / bwd partial sums
  const float* chan_part;  // fwd, optional: per-(64-row block, channel) partials (mean, M2) emitted by the producing convolutions
  int part_ld;             //   (CF_STATS), [B*HW/64][part_ld][2], already offset to channel 0 of x: replaces the statistics pass
  int B, HW, C, G;
  float eps;
  int silu;
  // backward only
  const bf16_t* dy; int dy_ld;
  bf16_t* dx; int dx_ld;
  int accumulate;      // dx += result
};
// Both launchers return hipErrorInvalidValue in front of any launch (and of any division by G) for: G, C, HW or B <= 0, B > 65535 (the
// images are the grid's y extent), C % 8, C % G, a row stride (x_ld, y_ld / dy_ld, dx_ld) that is no multiple of 8, chan_part with HW % 64.
size_t groupnorm_scratch_bytes(int B, int G);
hipError_t launch_groupnorm_fwd(const GroupNormParams& p, hipStream_t stream);
hipError_t launch_groupnorm_bwd(const GroupNormParams& p, hipStream_t stream);

// ----------------------------------------------------------------------------------------------
// K4: LayerNorm over the channel dim of [M, C] bf16 rows.
// ----------------------------------------------------------------------------------------------
struct LayerNormParams {
  const bf16_t* x; int x_ld;
  bf16_t* y; int y_ld;
  const float* gamma; const float* beta;
  float* stats;        // [M][2] mean, rstd
  int M, C; float eps;
  const float* rowpart; int rowpart_ld, spans;   // fwd, y == null: statistics only -- from the producing GEMM's row partials when given
                                                 // ([M][rowpart_ld][2] (sum, sum^2) over `spans` column spans), else from x
  const bf16_t* dy; int dy_ld;
  bf16_t* dx; int dx_ld;
  int accumulate;
};
// hipErrorInvalidValue in front of any launch for: M or C <= 0, C % 8, C > 2048, a row stride that is no multiple of 8 (y_ld only when y
// is given); forward with neither y nor stats, row partials with spans < 1 or rowpart_ld < spans; backward without stats.
hipError_t launch_layernorm_fwd(const LayerNormParams& p, hipStream_t stream);
hipError_t launch_layernorm_bwd(const LayerNormParams& p, hipStream_t stream);

// ----------------------------------------------------------------------------------------------
// K5: flash attention forward / backward. Q rows [B*Nq, ldq], head h at column h*D.
// ----------------------------------------------------------------------------------------------
struct AttnParams {
  const bf16_t* q; const bf16_t* k; const bf16_t* v;
  bf16_t* o; float* lse;                    // lse [B][H][Nq] (natural log domain, of scaled scores)
  int ldq, ldk, ldv, ldo;
  int B, H, Nq, Nk, D;
  float scale;
  // backward
  const bf16_t* d_o; int lddo;
  bf16_t* dq; bf16_t* dk; bf16_t* dv;       // dk/dv may be null (cross attention: dQ only)
  int lddq, lddk, lddv;
  float* delta;                             // [B][H][Nq] scratch: rowsum(dO*O)
  int q_prescaled;                          // Q already carries 1/sqrt(D) * log2(e) (folded into the to_q weights): scores are log2-domain; pass scale = ln 2
  int causal;                               // forward only: key j visible to query i iff j <= i (CLIP text encoder)
  int pv_fp8;                               // forward only, D = 64: P.V on the block-scaled fp8 MFMA (e4m3 probabilities and values)
  int no_shortk;                            // diagnostics: keep <= 80-key launches on the streaming forward (accuracy A/B inside one process)
};
// Scratch a launch may use for the GEMM route (wide heads, d >= 256: the AutoencoderKL mid-block attention, attention_gemm.hip, with a
// materialised N x N score matrix per image).  workspace: attention_gemm_workspace() bytes per image; with more, single-head layers run
// up to 8 images per launch (grouped GEMMs); tap1x1: device int holding the 1x1 tap ((32 << 6) | 32); partial: split-K scratch of
// launch_conv_gemm.  Empty (all zero): the flash kernels only -- what the engine passes for cross-attention.
struct AttnScratch {
  void* workspace; size_t workspace_bytes;
  const int* tap1x1;
  float* partial; size_t partial_cap;
};
// The one entry: plans (attention.hip: attention_plan -- GEMM route when the scratch allows it, else short keys, fp8, LDS-DMA staged,
// register-staged) and launches.  hipErrorInvalidValue and nothing launched for a problem the planner refuses.
hipError_t launch_attention(const AttnParams& p, const AttnScratch& scratch, bool bwd, hipStream_t stream);
// The same decision without a launch (no device access; the pointers are only tested for null): returns the route (ATTN_* of
// attention_dispatch.h, -1 refused) and fills out[26] = {route, head dim of the form, QT, KT, DSPLIT (backward: of the dQ kernel), KTW, QTL
// (dK/dV kernel, 0 when it does not run), waves, bits (1 lazy reference, 2 prescaled backward, 4 causal, 8 fp8), images per GEMM group,
// launches, then (grid x, y, z, block, dynamic LDS bytes) of each}.  The GEMM route reports route and group only.
int attention_plan_query(const AttnParams& p, size_t workspace_bytes, bool bwd, int* out);
// scratch_tmp bytes the engine has to offer an attention op so that the launch takes the route it can (0: none needed)
size_t attention_scratch_bytes(int B, int heads, int Nq, int Nk, int D, bool causal, bool cross, bool want_grad);
// the flash kernels only (empty scratch) ...
hipError_t launch_attention_fwd(const AttnParams& p, hipStream_t stream);
hipError_t launch_attention_bwd(const AttnParams& p, hipStream_t stream);
hipError_t launch_attention_delta(const AttnParams& p, hipStream_t stream);   // delta[b,h,q] = sum_d dO*O (first stage of the backward)
// ... and the GEMM route or a refusal.  Same arguments / results as the flash launchers.
size_t attention_gemm_workspace(int Nq, int Nk, int D, int bwd);
hipError_t launch_attention_gemm_fwd(const AttnParams& p, void* workspace, size_t workspace_bytes, const int* tap1x1, float* partial, size_t partial_cap, hipStream_t stream);
hipError_t launch_attention_gemm_bwd(const AttnParams& p, void* workspace, size_t workspace_bytes, const int* tap1x1, float* partial, size_t partial_cap, hipStream_t stream);

// ----------------------------------------------------------------------------------------------
// K6/K7/K9/K10/K12: small HBM-bound kernels.
// ----------------------------------------------------------------------------------------------
// The vectorised row kernels (launch_add / copy / mask / maxpool3x3s2* in both formats, sumpool2x2, geglu_bwd) move 16-byte vectors of
// V elements (8 bf16, 4 fp32: Row<T> in common.h): C (F) and every row stride must be multiples of V, the max pools also need even H and
// W (they pool to H / 2 x W / 2); anything else is hipErrorInvalidValue and nothing is launched.  Row base pointers must be 16-byte
// aligned (not checked: a column view has to start at a multiple of V channels).  The *_f32 forms of these kernels are declared with the
// fp32 guide below; both formats are instances of one kernel each (elementwise.hip).
// NCHW fp32 [B,C,H,W] -> NHWC bf16 [B*H*W, ld] (channels >= C zero-filled up to Cpad); dup copies
// the batch twice (CFG: cat[z, z]).  scale multiplies.
// cot_mul (here and below): a device scalar the values are multiplied by on top of `scale`, or null -- the cotangent scale of the fp16
// build at the entry of a reverse program, its inverse at the exit (launch_cot_scale); the bf16 build does not read it
hipError_t launch_nchw_f32_to_nhwc_bf16(const float* src, bf16_t* dst, int B, int C, int H, int W, int Cpad, int ld,
                                        int dup, float scale, hipStream_t s, const float* cot_mul = nullptr);
// NHWC (bf16 or fp32) [B*H*W, ld] -> NCHW fp32 [B,C,H,W];  out = in * scale + shift, optional clamp to [lo, hi]
hipError_t launch_nhwc_to_nchw_f32(const void* src, int src_f32, float* dst, int B, int C, int H, int W, int ld,
                                   float scale, float shift, int clamp, float lo, float hi, hipStream_t s, const float* cot_mul = nullptr);
// The sampler step (sampler_step.hip; generate_data.py:116-119 is its epsilon / DDIM mode): CFG mix, optional CFG rescale phi (Lin et al.
// 2023; diffusers rescale_noise_cfg), the scheduler update, and its VJP.
//   m = u + s (c - u),  m^ = m (phi sigma_c / sigma_m + 1 - phi) per image,  x0 = A_z z + A_m m^,  z' = B_z z + B_m m^ + c2m (x0 - x0_prev)
// Modes, chosen by the launchers from the fields below and from nothing else:
//   (prediction_type 0, phi 0)   the division form x0 = (z - sqrt(1-a) m) / sqrt a, z' = sqrt a' x0 + sqrt(1-a') m on coef; lin, stats and
//                                part are not read
//   every other (type, phi)      the linear form on lin
//   phi != 0                     stats [B][8] receives {k, sigma_c, sigma_m, mean_c, mean_m, N, phi} (kept for the backward), part is
//                                scratch of sampler_step_scratch_floats(B, HW) floats; the backward re-reads m2 of that step
//   x0_prev != null and c2m != 0 DPM-Solver++(2M), forward only (the guidance calls differentiate x0, which does not depend on the
//                                history): x0 is required and always written, and may alias x0_prev.  Otherwise x0_prev is not read
//   sigma != 0 and a noise source stochastic DDIM (eta > 0; forward only): coef / lin are the rows of rule 1 (sampler_step_row: sqrt(1-a')
//                                becomes d) and z' gains sigma n, n ~ N(0,1) per element: read from `noise` when it is given, otherwise
//                                generated in registers when rng_count > 0 -- element j = ch * HW + pix of row b takes lane j & 3 of Philox
//                                block j >> 2 of (rng_seed, rng_stream, unit id of row b - rng_row0), the bits launch_philox_units writes.
//                                The generated form steps rows [rng_row0, rng_row0 + rng_count) alone, rng_count <= DD_RNG_UNITS ids per
//                                launch: a larger batch is several launches over row ranges in order, and the one with rng_row0 == 0
//                                computes the statistics of phi != 0 for the whole batch.
//   both of the two above        SDE-DPM-Solver++(2M) (forward only): coef / lin are the rows of rule 2 and c2m is their c,
//                                z' = (the history step on those rows) + sigma n.  The generated form keeps its
//                                row ranges; every launch reads and writes its own rows only, so x0 may still alias x0_prev.
//                                With sigma == 0 or no source: the step above, nothing of this block is read.
//   halves == 1                  the CFG-free step of an engine that runs the UNet on the conditional prompt alone (dd_set_cfg_free): m2 is
//                                [B*HW, ld] and m = c -- no mix, coef[0] is not read; every mode above but the rescale, whose factor is
//                                identically 1 at m = c: phi != 0 is refused.  The backward writes g_m once, to rows [B*HW, ld] of g_m2.
// ld: a multiple of 8; C <= 8; B <= 65535; halves 1 or 2; anything else is hipErrorInvalidValue in front of any launch.  No atomics: bitwise
// deterministic.
#define DD_RNG_UNITS 16
struct RngUnits { unsigned lo[DD_RNG_UNITS], hi[DD_RNG_UNITS]; };
struct StepParams {
  const float* m2; int ld;             // model output, fp32 NHWC rows [2B*HW, ld], unconditional half first
  const float* z;                      // NCHW fp32 [B, C, HW], as x0_prev, z_prev and x0
  const float* x0_prev; float c2m;     // history and c of this step (StepRow::c2m)
  float* z_prev; float* x0;            // x0 may be null in a first-order step
  int B, C, HW;
  const float* coef;                   // device: {guidance_scale, sqrt_a_t, sqrt_1m_a_t, sqrt_a_prev, sqrt_1m_a_prev}
  const float* lin;                    // device: {A_z, A_m, B_z, B_m} (StepRow::lin)
  int prediction_type; float phi;      // 0 epsilon, 1 v_prediction, 2 sample; CFG rescale
  float* stats; float* part;
  const float* noise; float sigma;     // eta > 0 / SDE: explicit step noise NCHW fp32 [B, C, HW] (or null: generated) and sigma of this step
  uint64_t rng_seed; int rng_stream;   // the generated form: Philox key and stream (16 + step index)
  RngUnits rng_ids; int rng_count, rng_row0;
  int halves = 2;                      // 2: the CFG pair above.  1 (CFG-free): m2 is [B*HW, ld], the conditional output alone -- see below
};
// The host numbers of step i of an n-step schedule under one rule, from alphas_cumprod at step i - 1, at step i and at its previous
// timestep; formed in double, each float rounded once.  One function states them for every mode:
//   lin   {A_z, A_m, B_z, B_m} of the linear form, B_z / B_m on d in place of sqrt(1-a')
//   d     what the direction term keeps of the noise level 1 - a': coef[4] of the division form.  sqrt(1-a') under rule 0
//   sigma the scale of the fresh noise, d^2 + sigma^2 = 1 - a'.  0.0f under rule 0
//   c2m   c of the second-order step, c = sqrt(a') (1 - e^-h') / (2 r) with h' = h (rules 0, 1) or (1 + s) h (rule 2); exactly 0 for the
//         first and the last step and wherever it is undefined
// rule 1 (DDIM with eta = s, diffusers DDIMScheduler.step): sigma = s sqrt((1-a')/(1-a) (1-a/a')), d = sqrt(max(0, 1 - a' - sigma^2)).
// rule 2 (SDE-DPM-Solver++(2M), k-diffusion sample_dpmpp_2m_sde's eta = s; s = 1: diffusers sde-dpmsolver++): h = lambda(a') - lambda(a),
// d = sqrt(1-a') e^(-s h), sigma = sqrt(1-a') sqrt(-expm1(-2 s h)); a' = 1: d = sigma = 0; a' = a: (sqrt(1-a'), 0.0f); a = 0: (0, sqrt(1-a')).
// s = 0 under rule 1 or 2 gives the floats of rule 0 bit for bit.
// Returns 0; -1 refused in front of the arithmetic, *out untouched: s outside [0, 1] under rule 1 or 2, then an unknown prediction type or
// a singular step (a <= 0 for epsilon, a >= 1 for sample); -2 a row of rule 1 or 2 that is not finite, which *out then holds.  Rule 0
// does not look: its row at a = 1e-80 is {inf, -inf, inf, -inf} with 0.
struct StepRule { int prediction_type; int noise; double s; };      // noise: 0 none, 1 DDIM eta, 2 SDE-DPM-Solver++(2M); s = eta or sde_eta
struct StepRow { float lin[4]; float d; float sigma; float c2m; };
int sampler_step_row(const StepRule& r, int i, int n, double a_before, double a, double a_prev, StepRow* out);
size_t sampler_step_scratch_floats(int B, int HW);
// HOST unit_ids[0, B) in ranges of DD_RNG_UNITS, the most one launch carries: f(ids, first row, count) per range, in order; the first
// error ends the walk
template <class F>
hipError_t for_rng_unit_ranges(const uint64_t* unit_ids, int B, F f) {
  for (int r0 = 0; r0 < B; r0 += DD_RNG_UNITS) {
    RngUnits ids{};
    const int cnt = B - r0 < DD_RNG_UNITS ? B - r0 : DD_RNG_UNITS;
    for (int k = 0; k < cnt; ++k) { ids.lo[k] = (unsigned)unit_ids[r0 + k]; ids.hi[k] = (unsigned)(unit_ids[r0 + k] >> 32); }
    const hipError_t e = f(ids, r0, cnt);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
hipError_t launch_sampler_step(const StepParams& p, hipStream_t s);
// the generated form for a whole batch: unit_ids HOST [p.B], read before the call returns; DD_RNG_UNITS rows per launch (p.rng_ids,
// rng_count and rng_row0 are filled here).  With sigma == 0 this is launch_sampler_step(p).
hipError_t launch_sampler_step_units(const StepParams& p, const uint64_t* unit_ids, hipStream_t s);
// VJP of step p in (x0, z'): g_x0, g_zprev NCHW fp32 (either may be null) -> g_z NCHW fp32 (the direct path) and g_m2, bf16 NHWC rows
// [halves*B*HW, ld] with every column written (padding = 0).  p.z, p.x0_prev, p.z_prev and p.x0 are not used.  See DESIGN.md / SURVEY appendix A
hipError_t launch_sampler_step_bwd(const StepParams& p, const float* g_x0, const float* g_zprev, bf16_t* g_m2, float* g_z, hipStream_t s);
// backward of cat[z, z] + NCHW->NHWC: g_z[b,c,pix] (+)= gin[b*HW+pix, c] + gin[(B+b)*HW+pix, c]   (halves = 2), or of the plain
// layout change when the UNet input itself is not duplicated (halves = 1: the two CFG halves share their prefix, engine.cpp)
hipError_t launch_dup_bwd(const bf16_t* gin, int ld, float* g_z, int B, int C, int HW, int accumulate, int halves, hipStream_t s,
                          const float* cot_mul = nullptr);
// y = dy * (mask > 0)  (ReLU backward)
hipError_t launch_mask_bf16(const bf16_t* dy, int ldd, const bf16_t* mask, int ldm, bf16_t* y, int ldy, int M, int C,
                            hipStream_t s);
// add_noise: out = sa * x + sb * n   (fp32, n elements), coefficients from device memory {sa, sb}
hipError_t launch_axpby(const float* x, const float* n, float* out, size_t count, const float* coef_dev, hipStream_t s);
// Counter-based noise (rng.hip): Philox4x32-10, key = seed, counter = (j / 4, rng_stream, unit id lo, unit id hi) for element j of a
// unit; up to DD_RNG_UNITS unit ids travel in the kernel arguments (nothing of the caller's is referenced after the launch).
//   launch_philox_units    : out [count, n_per_unit] = the values of `rng_stream` (0, 1, 3: N(0,1) by Box-Muller; 2: U[0,1);
//                            DD_RNG_STEP_STREAM + i: N(0,1), the noise of step i under eta > 0; 4-15 reserved and refused)
//   launch_philox_add_noise: out [count, C, HW] = sa * x + sb * (n + 0.1 * o_c) with n from stream 0 and, when offset_noise, o_c from
//                            stream 1 at channel c; coef_dev = {sa, sb} as launch_axpby -- bit for bit what launch_axpby gives on the
//                            tensors of launch_philox_units
#define DD_RNG_STEP_STREAM 16
#define DD_RNG_STEP_STREAMS 4096
inline bool rng_stream_ok(int st) { return (st >= 0 && st <= 3) || (st >= DD_RNG_STEP_STREAM && st < DD_RNG_STEP_STREAM + DD_RNG_STEP_STREAMS); }
hipError_t launch_philox_units(const RngUnits& ids, int count, uint64_t seed, int rng_stream, int64_t n_per_unit, float* out, hipStream_t s);
hipError_t launch_philox_add_noise(const RngUnits& ids, int count, uint64_t seed, const float* x, float* out, int C, int HW, int offset_noise,
                                   const float* coef_dev, hipStream_t s);
// 2x2 sum pooling of NHWC bf16 (backward of the fused nearest-2x upsample): [B,2H,2W,C] -> [B,H,W,C]
hipError_t launch_sumpool2x2(const bf16_t* src, int src_ld, bf16_t* dst, int dst_ld, int B, int H, int W, int C,
                             int accumulate, hipStream_t s);
// y = a + b (bf16 rows), used where a fan-in cannot be fused into an epilogue
hipError_t launch_add_bf16(const bf16_t* a, int lda, const bf16_t* b, int ldb, bf16_t* y, int ldy, int M, int C,
                           hipStream_t s);
// copy rows (bf16) with strides
hipError_t launch_copy_bf16(const bf16_t* a, int lda, bf16_t* y, int ldy, int M, int C, hipStream_t s);
// GEGLU backward: raw packed [M, 2F] (16-col groups hidden|gate), dout [M, F] -> draw [M, 2F] packed
hipError_t launch_geglu_bwd(const bf16_t* raw, int ld_raw, const bf16_t* dout, int ld_dout, bf16_t* draw, int ld_draw,
                            int M, int F, hipStream_t s);
// max pool 3x3 stride 2 pad 1 NHWC bf16, and its backward (recomputes the argmax: first max in scan order)
hipError_t launch_maxpool3x3s2(const bf16_t* x, bf16_t* y, int B, int H, int W, int C, hipStream_t s);
hipError_t launch_maxpool3x3s2_bwd(const bf16_t* x, const bf16_t* dy, bf16_t* dx, int B, int H, int W, int C,
                                   hipStream_t s);
// bicubic (A=-0.75, align_corners=False, no antialias) NHWC: src [B,Hs,Ws,ld_s] (C real channels) -> dst [B,Hd,Wd,ld_d]
// channels >= C in dst are zero-filled up to Cpad.
hipError_t launch_bicubic(const bf16_t* src, int ld_s, bf16_t* dst, int ld_d, int B, int Hs, int Ws, int Hd, int Wd, int C,
                          int Cpad, hipStream_t s);
// transpose of the above: dsrc [B,Hs,Ws,C] (+)= sum of taps of ddst
hipError_t launch_bicubic_bwd(const bf16_t* ddst, int ld_d, bf16_t* dsrc, int ld_s, int B, int Hs, int Ws, int Hd, int Wd,
                              int C, hipStream_t s);
// global average pool [B, HW, C] bf16 -> f [B, C] fp32 ; backward broadcasts g/HW as bf16
hipError_t launch_gap(const bf16_t* x, int ld, float* f, int B, int HW, int C, hipStream_t s);
hipError_t launch_gap_bwd(const float* gf, bf16_t* dx, int ld, int B, int HW, int C, const bf16_t* mask, int mask_ld,
                          hipStream_t s);
// energy (generate_data.py:707-717 / 747-759) and its gradient wrt f.
//   f [B,D] fp32, Pc [Ccls,D], Pg [Ccls,K,D], targets [B] int32. normalize: direct-guidance L2-normalise first.
//   E_i = gs*||f_i-pc|| + ls*||f_i-pg*||;  score_out[0] += weight * sum_i w_i E_i;  gf [i,:] = weight * w_i * dE_i/df_i
//   w_i = sample_w[i] (device [B]) or 1/B when null: the reference's `.mean()` runs over its train_batch_size group
//   (:709-719, :750-760), which the caller expresses as w_i = 1/|group of i| when it packs several groups into one engine batch.
//   image_scores (device [B], may be null): image_scores[i] += weight * E_i.
hipError_t launch_energy(const float* f, const float* Pc, const float* Pg, const int* targets, int B, int D, int K,
                         float gs, float ls, int use_c, int use_g, int normalize, float weight, const float* sample_w,
                         float* score_out, float* image_scores, float* gf, hipStream_t s);
// transform guidance update (generate_data.py:696, 721-728): per (b,c): ge = sum_hw g*z, gb = sum_hw g;
//   e -= rho*ge, b -= rho*gb ; z_out = clamp(z*(1+e)+b, z-c, z+c) (lower bound first)
hipError_t launch_affine(const float* z, const float* e, const float* b, float* out, int BC, int HW, hipStream_t s);
hipError_t launch_transform_update(const float* z, const float* g, const float* e, const float* b, float* z_out, int BC,
                                   int HW, float rho, float c, hipStream_t s);
// out = a - rho * g  (direct guidance :762)
hipError_t launch_sub_scaled(const float* a, const float* g, float* out, size_t n, float rho, hipStream_t s);
// NHWC bf16 [M, ld] (first C channels) -> NCHW fp32, used for gradients wrt latents
// fp32 -> bf16 pack rows (weights upload helpers)
hipError_t launch_f32_to_bf16(const float* src, bf16_t* dst, size_t n, hipStream_t s, const float* cot_mul = nullptr);
#ifdef DD_ACT_F16
// The cotangent scale of the fp16 build (common.h: CotScale): scale2 = {s, 1 / s}, s the power of two that puts the absolute maximum of
// x[r * ld + c] (r < rows, c < C; and of x2 likewise, or null) into [2^7, 2^8), 1 for an all-zero cotangent.  Two stages, no atomics;
// part: cot_scale_scratch_floats() floats.  launch_cot_mul: x *= *mul in place.
size_t cot_scale_scratch_floats();
hipError_t launch_cot_scale(const float* x, size_t rows, int C, int ld, const float* x2, size_t rows2, int C2, int ld2, float* part, float* scale2,
                            hipStream_t s);
hipError_t launch_cot_mul(float* x, size_t rows, int C, int ld, const float* mul, hipStream_t s);
#endif
// setup-time fp32 linear: y = act(x) W^T + b (time-embedding tables)
hipError_t launch_linear_f32(const float* x, const float* W, const float* b, float* y, int M, int N, int K, int silu_in, hipStream_t s);
hipError_t launch_fill_f32(float* dst, float v, size_t n, hipStream_t s);
// SDXL added conditioning (setup-time, fp32): sinusoidal embedding of n scalars (diffusers Timesteps: flip_sin_to_cos, shift 0) into
// out[i*ld + off .. + dim); out[(s*nb + b), :] = a[s, :] + v[b, :]
hipError_t launch_sinusoid_f32(const float* x, float* out, int n, int dim, int ld, int off, int flip, hipStream_t s);
hipError_t launch_add_outer_f32(const float* a, const float* v, float* out, int ns, int nb, int cols, hipStream_t s);
// y[r, c] += v[c]  (fp32 rows; setup-time: the per-timestep bias tables)
hipError_t launch_add_rowvec_f32(float* y, const float* v, int rows, int cols, hipStream_t s);
// (x/2+0.5).clamp(0,1)*255+0.5 -> uint8 HWC (output stage, generate_data.py:1227 + save_image quantisation)
hipError_t launch_to_uint8(const float* nchw, uint8_t* hwc, int B, int C, int H, int W, hipStream_t s);

// f-2, the stage before the loop (dataloader.py:633-661, 750-811): CLIP token + position embedding gather, CLIP MLP activation
// (kind 0 quick_gelu, 1 erf-GELU), DiagonalGaussian sample * scaling_factor from fp32 NHWC moments, bf16 rows -> fp32 rows
hipError_t launch_clip_embed(const int* ids, const float* tok, const float* pos, bf16_t* out, int ld, int rows, int T, int C, int vocab,
                            hipStream_t s);
hipError_t launch_act_bf16(const bf16_t* x, int ldx, bf16_t* y, int ldy, int M, int C, int kind, hipStream_t s);
// the open_clip ViT guide (model_utils.py:80-87): GELU / quick_gelu backward, non-overlapping patch embedding as a GEMM (image fp32
// NHWC -> rows [B*(S/p)^2, C*p*p], k = (c, iy, ix)) and its transpose, class token + positional embedding, class-token selection
hipError_t launch_act_bwd_bf16(const bf16_t* x, int ldx, const bf16_t* dy, int ldd, bf16_t* dx, int ldo, int M, int C, int kind, int accumulate,
                               hipStream_t s);
hipError_t launch_patchify(const float* img, int ld, bf16_t* out, int B, int S, int p, int C, hipStream_t s);
hipError_t launch_patchify_bwd(const bf16_t* gout, float* gimg, int ld, int B, int S, int p, int C, hipStream_t s);
hipError_t launch_vit_embed(const bf16_t* patches, int ldp, const float* cls, const float* pos, bf16_t* out, int ldo, int B, int np, int W,
                            hipStream_t s);
hipError_t launch_vit_embed_bwd(const bf16_t* gout, int ldo, bf16_t* gp, int ldp, int B, int np, int W, hipStream_t s);
hipError_t launch_select_rows(const bf16_t* x, int ldx, bf16_t* y, int ldy, int B, int stride, int C, hipStream_t s);
hipError_t launch_select_rows_bwd(const bf16_t* dy, int ldy, bf16_t* dx, int ldx, int B, int stride, int C, int accumulate, hipStream_t s);
hipError_t launch_vae_sample(const float* moments, int ld, const float* noise, float* latents, float* moments_out, int B, int C, int HW,
                             float scale, hipStream_t s);
hipError_t launch_rows_bf16_to_f32(const bf16_t* x, int ld, float* y, int M, int C, hipStream_t s);
hipError_t launch_clip_pool_project(const int* ids, const bf16_t* x, int ld, const float* W, float* out, int n, int T, int C, int Pd, hipStream_t s);

// ----------------------------------------------------------------------------------------------
// The guide network in exact fp32: implicit-GEMM convolution on v_mfma_f32_32x32x2_f32 (guide_f32.hip) and the fp32
// forms of the guide's side kernels (elementwise.hip).  Same tap-table / stride / dilated-gather conventions as ConvGemmParams.
// ----------------------------------------------------------------------------------------------
struct ConvF32Params {
  const float* x;       // input activations, NHWC fp32, row stride x_ld (multiple of 4)
  const float* w;       // packed weights [N][K] fp32, k = (tap, cin), K % 16 == 0 (zero padded)
  const int* taptab;
  float* y;             // output fp32, row stride y_ld
  const float* bias;    // [N] or null
  const float* res;     // residual (CF_RES); may alias y (accumulating dgrad)
  const float* mask;    // CF_MASK: multiply by (mask[m, n] > 0)
  int x_ld, y_ld, res_ld, mask_ld;
  int B, H, W, Ho, Wo, stride, shift, parity;
  int cin, ntaps;       // channels per tap (multiple of 4; of 16 when groups > 1), taps
  int M, N, K;
  int groups, cpg_in, cpg_out;   // groups > 1: output column n reads K-channels [g*cpg_in, (g+1)*cpg_in), g = n / cpg_out
  int flags;            // CF_BIAS | CF_RES | CF_RELU | CF_MASK
};
hipError_t launch_conv_f32(const ConvF32Params& p, hipStream_t s);
hipError_t launch_add_f32(const float* a, int lda, const float* b, int ldb, float* y, int ldy, int M, int C, hipStream_t s);
hipError_t launch_copy_f32(const float* a, int lda, float* y, int ldy, int M, int C, hipStream_t s);
// y = dy * (mask > 0 [&& mask < hi when hi > 0])   (ReLU / ReLU6 backward from the stored forward output)
hipError_t launch_mask_f32(const float* dy, int ldd, const float* mask, int ldm, float* y, int ldy, int M, int C, float hi, hipStream_t s);
hipError_t launch_maxpool3x3s2_f32(const float* x, float* y, int B, int H, int W, int C, hipStream_t s);
hipError_t launch_maxpool3x3s2_bwd_f32(const float* x, const float* dy, float* dx, int B, int H, int W, int C, hipStream_t s);
// src fp32 NHWC [B,Hs,Ws,ld_s] -> dst fp32 [B,Hd,Wd,ld_d]; the transpose writes bf16 rows (dsrc_bf16) or fp32
hipError_t launch_bicubic_f32(const float* src, int ld_s, float* dst, int ld_d, int B, int Hs, int Ws, int Hd, int Wd, int C, int Cpad,
                              hipStream_t s);
hipError_t launch_bicubic_bwd_f32(const float* ddst, int ld_d, void* dsrc, int dsrc_bf16, int ld_s, int B, int Hs, int Ws, int Hd, int Wd,
                                  int C, hipStream_t s, const float* cot_mul = nullptr);
// global average (or max, model_utils.py:34-35) pool of fp32 rows -> f [B, C]; argmax [B, C] only for the max form
hipError_t launch_gap_f32(const float* x, int ld, float* f, int* argmax, int B, int HW, int C, int use_max, hipStream_t s);
hipError_t launch_gap_bwd_f32(const float* gf, float* dx, int ld, int B, int HW, int C, const int* argmax, hipStream_t s);
hipError_t launch_nchw_to_nhwc_f32(const float* src, float* dst, int B, int C, int H, int W, int Cpad, int ld, hipStream_t s);

// ----------------------------------------------------------------------------------------------
// host-side weight packing (weights.cpp)
// ----------------------------------------------------------------------------------------------
struct PackedConv {
  int N, K, cin, ntaps;   // GEMM N, padded K, padded channels per tap, taps
};
// mode 0: forward conv/linear weights [Cout][Cin][KH][KW] -> [N=Cout][K], taps (ky-pad, kx-pad)
// mode 1: input-gradient (dgrad) weights               -> [N=Cin][K=(tap, cout)], taps (pad-ky, pad-kx)
// geglu: the Cout dimension is permuted into 32-wide (16 hidden | 16 gate) groups (see CF_GEGLU)
PackedConv pack_conv_shape(int Cout, int Cin, int KH, int KW, int mode);
void pack_conv_weight(const float* w, int Cout, int Cin, int KH, int KW, int pad, int mode, int geglu, bf16_t* wp, int* taptab);
// fp32 packing for the guide network (guide_f32.hip): cin padded to 4 (16 when groups > 1), K padded to 16, k = (tap, cin);
// w is [Cout][Cin/groups][KH][KW] (torch grouped-conv layout), packed as the dense block-diagonal matrix
PackedConv pack_conv_shape_f32(int Cout, int Cin, int KH, int KW, int mode, int groups);
void pack_conv_weight_f32(const float* w, int Cout, int Cin, int KH, int KW, int pad, int mode, int groups, float* wp, int* taptab);
int geglu_perm(int packed_index, int F);  // packed column -> original row of the [2F] projection
bf16_t host_f2bf(float f);
float host_bf2f(bf16_t v);
