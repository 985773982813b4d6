/* distdiff_hip_ops.h — op-level C ABI of libdistdiff_hip.so (diagnostic / unit-test surface).
 *
 * Each entry point enqueues ONE hand-written gfx950 kernel family on the caller's HIP stream with
 * plain device pointers; the parity tests in tests/ call these against the CPU oracle. The
 * production boundary (the reference's sampler functions, generate_data.py:109-121, 687-767) is
 * include/distdiff_hip.h. All functions return 0 on success or a hipError_t value.
 *
 * Reference operation each one replaces (file:line in haoweiz23/DistDiff):
 *   dd_op_conv_gemm      diffusers Conv2d / Linear / timm conv+BN inside unet(), vae.decode(), encode_image()
 *                        (generate_data.py:112, :701, :705) and their input-gradients (:721, :761)
 *   dd_op_groupnorm_*    GroupNorm(+SiLU) in ResnetBlock2D / Transformer2D / VAE decoder (:112, :701)
 *   dd_op_layernorm_*    LayerNorm in BasicTransformerBlock (:112)
 *   dd_op_attention_*    scaled-dot-product attention (self, cross, VAE mid block) (:112, :701)
 *   dd_op_sampler_step*  classifier-free guidance + DDIMScheduler.step (:116-119) for every prediction type, with optional CFG rescale
 *                        and, as dd_op_sampler_step_2m, the step of DPM-Solver++(2M), as dd_op_sampler_step_n the stochastic step
 *                        of eta > 0, as dd_op_sampler_step_2m_n the step of SDE-DPM-Solver++(2M) (all beyond the reference, which builds an
 *                        epsilon DDIMScheduler); dd_op_cfg_ddim* are its (epsilon, no rescale) mode under their first names
 *   dd_op_bicubic*       F.interpolate(..., (224,224), 'bicubic') (:704, :745)
 *   dd_op_conv_f32       timm conv+BN(+ReLU) of image_encoder.encode_image and its input-gradient in exact fp32
 *                        (model_utils.py:29-41; generate_data.py:705, :721, :746, :761): v_mfma_f32_32x32x2_f32
 *   dd_op_energy         prototype energy terms (:707-717, :747-759)
 *   dd_op_transform_update  SGD step on (e, b), re-affine, linfball_proj (:721-728, :124-137)
 */
#ifndef DISTDIFF_HIP_OPS_H
#define DISTDIFF_HIP_OPS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* parameter blocks are the POD structs of distdiff_amd/csrc/kernels.h, passed by pointer */
struct ConvGemmParams;
struct GroupNormParams;
struct LayerNormParams;
struct AttnParams;
struct ConvF32Params;

/* taptab contract: entry t = ((dy + 32) << 6) | (dx + 32).  A launch with ONE tap, stride 1 and an output of the input's size is a
 * pointwise (1x1 / linear) layer and must carry the centre tap (dy = dx = 0) -- the persistent kernels skip the table for it.  The
 * entry point is stream-asynchronous and does not read device memory: the owner of the table checks it on the host when the weights
 * are packed (distdiff_amd/ops.py raises on any other single tap). */
int dd_op_conv_gemm(const struct ConvGemmParams* p, size_t partial_cap_bytes, void* stream);
/* Which kernel dd_op_conv_gemm(p, partial_cap_bytes, .) would run, decided by the launcher's own code without launching anything (no
 * device access; the pointers are only tested for null): 0 the general implicit-GEMM kernels (conv_gemm_kernel / conv_gemm_big_kernel),
 * 1 conv_halo_kernel, 2 conv_halo_persist_kernel, 3 gemm_ws_kernel, 4 gemm_pps_kernel; DD_ERR_ARG (-1) for a problem the launcher refuses. */
int dd_op_conv_gemm_kind(const struct ConvGemmParams* p, size_t partial_cap_bytes);
/* The same dry decision with the form inside the kind: returns the kind and fills out4 = {kind, configuration of conv_gemm_big_kernel (0:
 * the small conv_gemm_kernel; 1 128 x 256, 2 256 x 160, 3 256 x 128 tiles on 8 waves; 4 128 x 160, 5 128 x 128 as two 4-wave workgroups
 * per CU), split-K (chunk split at the 8 x 8 halo level) the launch uses, 1 when the small kernel runs 256 x 64 instead of 128 x 128 tiles} */
int dd_op_conv_gemm_plan(const struct ConvGemmParams* p, size_t partial_cap_bytes, int* out4);
/* What the launch does beyond the output's bits when one of the halo 3x3 kernels runs the problem (the same dry decision: no device
 * access).  Returns 0 when the launcher would not run a halo kernel (a refused problem included), DD_ERR_ARG for a null argument, else 1
 * with out12 = {kind (1 | 2), tile form (1: 512 x 32 narrow, 2: 512 x 128, 4: 256 x 256, 5: 256 x 320, 6: 512 x 160), tile width and
 * height in output pixels, tiles per image row, tile rows per image, images per tile (4 at 8 x 8 images), halo address table in LDS
 * 0 / 1, dynamic LDS bytes, grid x, grid y (the chunk split), persistent kernel 0 / 1}.  Added without a version bump. */
int dd_op_conv_halo_plan(const struct ConvGemmParams* p, size_t partial_cap_bytes, int* out12);
/* Synchronous check of that contract against the DEVICE table (waits for the stream, copies the table back): 0 when every entry is in
 * range and a pointwise launch carries the centre tap.  For ABI users without a host copy of their tables; never called by the engine. */
int dd_op_conv_gemm_check(const struct ConvGemmParams* p, void* stream);
int dd_op_groupnorm_fwd(const struct GroupNormParams* p, void* stream);
int dd_op_groupnorm_bwd(const struct GroupNormParams* p, void* stream);
size_t dd_op_groupnorm_scratch_bytes(int B, int G);
int dd_op_layernorm_fwd(const struct LayerNormParams* p, void* stream);
int dd_op_layernorm_bwd(const struct LayerNormParams* p, void* stream);
int dd_op_attention_fwd(const struct AttnParams* p, void* stream);
int dd_op_attention_bwd(const struct AttnParams* p, void* stream);
/* wide heads (d >= 256, the AutoencoderKL mid-block attention): the same attention through GEMMs on a materialised N x N score
 * matrix per image.  workspace / workspace_bytes: device scratch of at least dd_op_attention_gemm_workspace() bytes (ONE image); given
 * k times that, single-head layers run up to min(k, 8) images per launch (grouped GEMMs); tap1x1: device int = (32 << 6) | 32;
 * partial / partial_cap: split-K scratch as for dd_op_conv_gemm. */
size_t dd_op_attention_gemm_workspace(int Nq, int Nk, int D, int bwd);
int dd_op_attention_gemm_fwd(const struct AttnParams* p, void* workspace, size_t workspace_bytes, const int* tap1x1, float* partial, size_t partial_cap, void* stream);
int dd_op_attention_gemm_bwd(const struct AttnParams* p, void* workspace, size_t workspace_bytes, const int* tap1x1, float* partial, size_t partial_cap, void* stream);
/* The one entry behind the four above: plans and launches the forward (bwd = 0) or the backward.  With workspace (as for
 * dd_op_attention_gemm_*) a problem the GEMM route takes runs there, everything else -- and everything when workspace is NULL -- on the
 * flash kernels: short keys, fp8 P.V, LDS-DMA staged, register-staged, in that order. */
int dd_op_attention(const struct AttnParams* p, void* workspace, size_t workspace_bytes, const int* tap1x1, float* partial, size_t partial_cap, int bwd, void* stream);
/* What dd_op_attention(p, a workspace of workspace_bytes, ...) would do, decided by the launcher's own planner without launching anything
 * (no device access; the pointers are only tested for null).  Returns the route -- 0 GEMM, 1 short-key, 2 LDS-DMA staged, 3
 * register-staged, 4 flash backward; DD_ERR_ARG (-1) for a problem the launcher refuses -- and fills out[26] = {route, head dim of the tile
 * form, QT, KT, DSPLIT (backward: of the dQ kernel), KTW, QTL (dK/dV kernel; 0 when it does not run), waves per workgroup, bits (1 lazy
 * reference, 2 prescaled backward, 4 causal, 8 fp8), images per GEMM group, launches, then (grid x, y, z, block, dynamic LDS bytes) of up to
 * three launches}.  The GEMM route reports route and group only. */
int dd_op_attention_plan(const struct AttnParams* p, size_t workspace_bytes, int bwd, int* out26);
/* Scratch (bytes of workspace) that lets dd_op_attention take the GEMM route for such an op on up to 8 images per launch; 0: no use for any */
size_t dd_op_attention_scratch_bytes(int B, int heads, int Nq, int Nk, int D, int causal, int cross, int want_grad);

/* fp32 implicit-GEMM convolution / dgrad of the guide network (guide_f32.hip) and its weight packing: w is
 * [Cout][Cin/groups][KH][KW] fp32 (torch grouped layout); out4 = {N, K, cin, ntaps}; wp may be NULL to query sizes */
int dd_op_conv_f32(const struct ConvF32Params* p, void* stream);
int dd_pack_conv_weight_f32(const float* w, int Cout, int Cin, int KH, int KW, int pad, int mode, int groups, float* wp, int* taptab,
                            int* out4);

/* host-side weight packing: returns N, K, cin, ntaps through out[4]; wp may be NULL to query sizes */
int dd_pack_conv_weight(const float* w_oihw, int Cout, int Cin, int KH, int KW, int pad, int mode, int geglu,
                        uint16_t* wp, int* taptab, int* out4);

int dd_op_nchw_f32_to_nhwc_bf16(const float* src, uint16_t* dst, int B, int C, int H, int W, int Cpad, int ld, int dup,
                                float scale, void* stream);
int dd_op_nhwc_to_nchw_f32(const void* src, int src_f32, float* dst, int B, int C, int H, int W, int ld, float scale,
                           float shift, int clamp, float lo, float hi, void* stream);
/* The sampler step: ONE operation (one forward kernel, one backward kernel; distdiff_amd/csrc/sampler_step.hip) behind the entry
 * points below, for every prediction_type (0 epsilon, 1 v_prediction, 2 sample; diffusers DDIMScheduler.step, eta = 0) with optional
 * classifier-free-guidance rescale (guidance_rescale = phi of Lin et al. 2023, diffusers rescale_noise_cfg) and optional second-order
 * term of DPM-Solver++(2M) (dd_set_schedule_s, solver 1; forward only):
 *   m = u + s (c - u),  m^ = m (phi std(c) / std(m) + 1 - phi) per image (unbiased std over the C*HW real elements),
 *   x0 = A_z z + A_m m^,  z' = B_z z + B_m m^ + c2m (x0 - x0_prev).
 * Modes, chosen from the arguments alone:
 *   (prediction_type 0, guidance_rescale 0)  evaluates x0 = (z - sqrt(1-a) m) / sqrt a, z' = sqrt a' x0 + sqrt(1-a') m on coef_dev =
 *       {s, sqrt a, sqrt(1-a), sqrt a', sqrt(1-a')}; lin_dev, stats and part may be NULL.  dd_op_cfg_ddim / dd_op_cfg_ddim_bwd are
 *       this mode and take only what it reads.
 *   every other (type, rescale)  evaluates the linear form on lin_dev = {A_z, A_m, B_z, B_m}, filled by dd_op_step_coefs (host, double
 *       arithmetic; -1 for an unknown type or a singular step: epsilon at a = 0, sample at a = 1) from alphas_cumprod at t and at the
 *       previous timestep; coef_dev[0] = s.
 *   guidance_rescale != 0  stats DEVICE [B][8] receives {k, std_c, std_m, mean_c, mean_m, N, phi} and is read again by the backward,
 *       part is DEVICE scratch of dd_op_sampler_step_scratch_floats(B, HW) floats, and the backward re-reads m2 (the forward's model
 *       output); all three may be NULL otherwise.
 *   x0_prev != NULL and c != 0 (dd_op_sampler_step_2m)  adds c (x0 - x0_prev); x0 is then required, is always written and may be x0_prev
 *       itself.  c = dd_op_step_coef_2m(i, n, a_before, a, a_prev) (host, double arithmetic, rounded once) from alphas_cumprod at step
 *       i - 1, at step i and at step i's previous timestep: with lambda(a) = ln(a / (1 - a)) / 2, h = lambda(a_prev) - lambda(a),
 *       r = (lambda(a) - lambda(a_before)) / h, c = sqrt(a_prev) (1 - e^-h) / (2 r); exactly 0.0f for i = 0, i = n - 1 and wherever a
 *       lambda or c is not finite.  With x0_prev NULL or c == 0 the history is not read and x0 may be NULL: dd_op_sampler_step is that call.
 *   sigma != 0 and a noise source (dd_op_sampler_step_n; forward only, no history)  adds sigma n: coef_dev[4] = d (division form) or
 *       lin_dev = the first four floats of dd_op_step_coefs_eta(type, a, a_prev, eta, out5) = {A_z, A_m, B_z, B_m, sigma} (host, double
 *       arithmetic; -1 as dd_op_step_coefs, for eta outside [0, 1] and for a result that is not finite; eta = 0: the floats of
 *       dd_op_step_coefs and sigma = 0.0f).  n is `noise` DEVICE NCHW fp32 [B, C, HW] when given; otherwise, with unit_ids HOST [B] (read
 *       before the call returns), it is generated in registers: element j = ch * HW + pix of row b is value j of
 *       dd_randn_units(seed, rng_stream, unit_ids[b]), rng_stream = 16 + step index -- the same bits, 16 rows per launch.  z' =
 *       (the step on those coefficients) + sigma * n: the product rounded, then the sum.  sigma == 0 or neither source: dd_op_sampler_step.
 * m2 fp32 rows [2B*HW, ld], unconditional half first; z, x0_prev, z', x0 and the cotangents NCHW fp32; g_m2 bf16 rows (every column
 * written, padding 0); g_x0 or g_zprev may be NULL.
 * Shapes: ld a multiple of 8, C <= 8, B <= 65535, for EVERY entry point; anything else returns hipErrorInvalidValue and launches
 * nothing.  (Up to ABI 9's first builds dd_op_cfg_ddim* ran a scalar kernel of their own that took any ld and C; no caller used one.)
 * Two-stage reductions in a fixed order, no atomics: the same call gives the same bits.  Which results are rounded once and which
 * twice is written out in the kernels' source and pinned by tests/test_sampler_step_bits_gpu.py. */
int dd_op_cfg_ddim(const float* eps2, int ld, const float* z, float* z_prev, float* x0, int B, int C, int HW,
                   const float* coef_dev, void* stream);
int dd_op_cfg_ddim_bwd(const float* g_x0, const float* g_zprev, uint16_t* g_eps2, int ld, float* g_z, int B, int C, int HW,
                       const float* coef_dev, void* stream);
int dd_op_step_coefs(int prediction_type, double a, double a_prev, float* out4);
size_t dd_op_sampler_step_scratch_floats(int B, int HW);
int dd_op_sampler_step(const float* m2, int ld, const float* z, float* z_prev, float* x0, int B, int C, int HW, const float* coef_dev,
                       const float* lin_dev, int prediction_type, float guidance_rescale, float* stats, float* part, void* stream);
int dd_op_sampler_step_bwd(const float* g_x0, const float* g_zprev, uint16_t* g_m2, int ld, float* g_z, int B, int C, int HW,
                           const float* coef_dev, const float* lin_dev, int prediction_type, float guidance_rescale, const float* m2,
                           const float* stats, float* part, void* stream);
float dd_op_step_coef_2m(int step_index, int n_steps, double a_before, double a, double a_prev);
int dd_op_sampler_step_2m(const float* m2, int ld, const float* z, const float* x0_prev, float c, float* z_prev, float* x0, int B, int C,
                          int HW, const float* coef_dev, const float* lin_dev, int prediction_type, float guidance_rescale, float* stats,
                          float* part, void* stream);
int dd_op_step_coefs_eta(int prediction_type, double a, double a_prev, double eta, float* out5);
int dd_op_sampler_step_n(const float* m2, int ld, const float* z, const float* noise, float sigma, uint64_t seed, int rng_stream,
                         const uint64_t* unit_ids, float* z_prev, float* x0, int B, int C, int HW, const float* coef_dev,
                         const float* lin_dev, int prediction_type, float guidance_rescale, float* stats, float* part, void* stream);
/* SDE-DPM-Solver++(2M) (dd_set_schedule_sde): history and noise in one step.  With s = sde_eta in [0, 1], h = lambda(a_prev) - lambda(a):
 *   dd_op_step_coefs_sde(type, a, a_prev, s, out5) = {A_z, A_m, B_z, B_m, sigma_n} with d = sqrt(1 - a_prev) e^(-s h) in the place of
 *       sqrt(1 - a_prev) (lin_dev = the first four floats; coef_dev[4] = d rounded once for the division form) and sigma_n =
 *       sqrt(1 - a_prev) sqrt(1 - e^(-2 s h)).  a_prev = 1: d = sigma_n = 0; a_prev = a: d = sqrt(1 - a_prev), sigma_n = 0.0f; a = 0:
 *       d = 0, sigma_n = sqrt(1 - a_prev).  -1 as dd_op_step_coefs, for s outside [0, 1] or not finite, and for a result that is not
 *       finite; s = 0: the floats of dd_op_step_coefs and 0.0f.
 *   dd_op_step_coef_2m_sde(i, n, a_before, a, a_prev, s, out): *out = sqrt(a_prev) (1 - e^(-(1 + s) h)) / (2 r), 0.0f exactly where
 *       dd_op_step_coef_2m is; returns -1 for s outside [0, 1] or not finite (and for out == NULL), else 0; s = 0: the float of
 *       dd_op_step_coef_2m.
 *   dd_op_sampler_step_2m_n: dd_op_sampler_step_2m and dd_op_sampler_step_n in one call, z' = (fma(B_z, t, B_m m^) + c (x0 - x0_prev))
 *       + sigma n, the product and the sum rounded separately.  With x0_prev NULL or c == 0 it is dd_op_sampler_step_n, with sigma == 0
 *       or no noise source dd_op_sampler_step_2m, bit for bit.  x0 may be x0_prev; the generated form takes 16 rows per launch and
 *       every launch touches its own rows only. */
int dd_op_step_coefs_sde(int prediction_type, double a, double a_prev, double sde_eta, float* out5);
int dd_op_step_coef_2m_sde(int step_index, int n_steps, double a_before, double a, double a_prev, double sde_eta, float* out);
int dd_op_sampler_step_2m_n(const float* m2, int ld, const float* z, const float* x0_prev, float c, const float* noise, float sigma,
                            uint64_t seed, int rng_stream, const uint64_t* unit_ids, float* z_prev, float* x0, int B, int C, int HW,
                            const float* coef_dev, const float* lin_dev, int prediction_type, float guidance_rescale, float* stats,
                            float* part, void* stream);
/* The CFG-free step (dd_set_cfg_free: the UNet runs on the conditional prompt alone), m = c:
 *   dd_op_sampler_step1: m1 fp32 rows [B*HW, ld], the conditional output -- there is no unconditional half and no mix, coef_dev[0] is
 *       not read (coef_dev may be NULL outside the division form, lin_dev inside it).  Every optional input of dd_op_sampler_step_2m_n
 *       with the same meaning and the same "modes chosen from the arguments alone": (prediction_type 0) the division form on
 *       coef_dev[1..4], every other type the linear form on lin_dev; x0_prev != NULL and c != 0 the second-order term; sigma != 0 with
 *       `noise` or unit_ids the stochastic step; both SDE-DPM-Solver++(2M).  No guidance_rescale / stats / part: the rescale factor is
 *       identically 1 at m = c.  z' and x0 are those of dd_op_sampler_step_2m_n on m2 = [c; c] at any finite s, bit for bit
 *       (fma(s, c - c, c) == c).
 *   dd_op_sampler_step1_bwd: g_m1 bf16 rows [B*HW, ld], g_m written once (every column written, padding 0) -- no (1 - s, s) split;
 *       g_z as dd_op_sampler_step_bwd.  g_m1 equals the conditional rows of dd_op_sampler_step_bwd at s = 1, bit for bit.
 * Shapes and refusals as above. */
int dd_op_sampler_step1(const float* m1, int ld, const float* z, const float* x0_prev, float c, const float* noise, float sigma,
                        uint64_t seed, int rng_stream, const uint64_t* unit_ids, float* z_prev, float* x0, int B, int C, int HW,
                        const float* coef_dev, const float* lin_dev, int prediction_type, void* stream);
int dd_op_sampler_step1_bwd(const float* g_x0, const float* g_zprev, uint16_t* g_m1, int ld, float* g_z, int B, int C, int HW,
                            const float* coef_dev, const float* lin_dev, int prediction_type, void* stream);
int dd_op_sumpool2x2(const uint16_t* src, int src_ld, uint16_t* dst, int dst_ld, int B, int H, int W, int C, int accumulate,
                     void* stream);
int dd_op_geglu_bwd(const uint16_t* raw, int ld_raw, const uint16_t* dout, int ld_dout, uint16_t* draw, int ld_draw, int M,
                    int F, void* stream);
int dd_op_maxpool3x3s2(const uint16_t* x, uint16_t* y, int B, int H, int W, int C, void* stream);
int dd_op_maxpool3x3s2_bwd(const uint16_t* x, const uint16_t* dy, uint16_t* dx, int B, int H, int W, int C, void* stream);
int dd_op_bicubic(const uint16_t* src, int ld_s, uint16_t* dst, int ld_d, int B, int Hs, int Ws, int Hd, int Wd, int C,
                  int Cpad, void* stream);
int dd_op_bicubic_bwd(const uint16_t* ddst, int ld_d, uint16_t* dsrc, int ld_s, int B, int Hs, int Ws, int Hd, int Wd, int C,
                      void* stream);
int dd_op_gap(const uint16_t* x, int ld, float* f, int B, int HW, int C, void* stream);
int dd_op_energy(const float* f, const float* Pc, const float* Pg, const int* targets, int B, int D, int K, float gs, float ls,
                 int use_c, int use_g, int normalize, float weight, float* score_out, float* gf, void* stream);
int dd_op_transform_update(const float* z, const float* g, const float* e, const float* b, float* z_out, int BC, int HW,
                           float rho, float c, void* stream);
int dd_op_affine(const float* z, const float* e, const float* b, float* out, int BC, int HW, void* stream);

/* ---- side kernels of the reverse programs (the launchers of distdiff_amd/csrc/kernels.h, one thin forward each) ----
 * bf16 rows [M, ld]: the 8-wide kernels (add, copy, mask, sumpool2x2, maxpool, geglu_bwd) refuse C or a row stride that is not a
 * multiple of 8, the max pools odd H / W (hipErrorInvalidValue, nothing is launched); the fp32 forms below the same with 4. */
int dd_op_mask_bf16(const uint16_t* dy, int ldd, const uint16_t* mask, int ldm, uint16_t* y, int ldy, int M, int C, void* stream);
int dd_op_add_bf16(const uint16_t* a, int lda, const uint16_t* b, int ldb, uint16_t* y, int ldy, int M, int C, void* stream);
int dd_op_copy_bf16(const uint16_t* a, int lda, uint16_t* y, int ldy, int M, int C, void* stream);
int dd_op_dup_bwd(const uint16_t* gin, int ld, float* g_z, int B, int C, int HW, int accumulate, int halves, void* stream);
int dd_op_gap_bwd(const float* gf, uint16_t* dx, int ld, int B, int HW, int C, const uint16_t* mask, int mask_ld, void* stream);
int dd_op_act_bf16(const uint16_t* x, int ldx, uint16_t* y, int ldy, int M, int C, int kind, void* stream);
int dd_op_act_bwd_bf16(const uint16_t* x, int ldx, const uint16_t* dy, int ldd, uint16_t* dx, int ldo, int M, int C, int kind,
                       int accumulate, void* stream);
int dd_op_patchify(const float* img, int ld, uint16_t* out, int B, int S, int p, int C, void* stream);
int dd_op_patchify_bwd(const uint16_t* gout, float* gimg, int ld, int B, int S, int p, int C, void* stream);
int dd_op_vit_embed(const uint16_t* patches, int ldp, const float* cls, const float* pos, uint16_t* out, int ldo, int B, int np, int W,
                    void* stream);
int dd_op_vit_embed_bwd(const uint16_t* gout, int ldo, uint16_t* gp, int ldp, int B, int np, int W, void* stream);
int dd_op_select_rows(const uint16_t* x, int ldx, uint16_t* y, int ldy, int B, int stride, int C, void* stream);
int dd_op_select_rows_bwd(const uint16_t* dy, int ldy, uint16_t* dx, int ldx, int B, int stride, int C, int accumulate, void* stream);
int dd_op_sub_scaled(const float* a, const float* g, float* out, size_t n, float rho, void* stream);
/* dd_op_energy with per-image weights w_i = sample_w[i] (device [B]; NULL: 1 / B) and image_scores[i] += weight * E_i (device [B] or NULL) */
int dd_op_energy_weighted(const float* f, const float* Pc, const float* Pg, const int* targets, int B, int D, int K, float gs, float ls,
                          int use_c, int use_g, int normalize, float weight, const float* sample_w, float* score_out,
                          float* image_scores, float* gf, void* stream);
/* fp32 rows (guide_f32.hip).  mask: y = dy * (mask > 0 [&& mask < hi when hi > 0]); gap: argmax only for the max form; gap_bwd: argmax
 * NULL = the average form; bicubic_bwd: dsrc is bf16 rows when dsrc_bf16, else fp32 */
int dd_op_mask_f32(const float* dy, int ldd, const float* mask, int ldm, float* y, int ldy, int M, int C, float hi, void* stream);
int dd_op_add_f32(const float* a, int lda, const float* b, int ldb, float* y, int ldy, int M, int C, void* stream);
int dd_op_copy_f32(const float* a, int lda, float* y, int ldy, int M, int C, void* stream);
int dd_op_maxpool3x3s2_f32(const float* x, float* y, int B, int H, int W, int C, void* stream);
int dd_op_maxpool3x3s2_bwd_f32(const float* x, const float* dy, float* dx, int B, int H, int W, int C, void* stream);
int dd_op_bicubic_f32(const float* src, int ld_s, float* dst, int ld_d, int B, int Hs, int Ws, int Hd, int Wd, int C, int Cpad,
                      void* stream);
int dd_op_bicubic_bwd_f32(const float* ddst, int ld_d, void* dsrc, int dsrc_bf16, int ld_s, int B, int Hs, int Ws, int Hd, int Wd, int C,
                          void* stream);
int dd_op_gap_f32(const float* x, int ld, float* f, int* argmax, int B, int HW, int C, int use_max, void* stream);
int dd_op_gap_bwd_f32(const float* gf, float* dx, int ld, int B, int HW, int C, const int* argmax, void* stream);
int dd_op_nchw_to_nhwc_f32(const float* src, float* dst, int B, int C, int H, int W, int Cpad, int ld, void* stream);

/* ---- test-only hooks into a dd_engine (include/distdiff_hip.h); no production caller ----
 * debug introspection of the op graph: host copy of an activation or gradient of tensor idx (negative: from the end, -1 = the
 * program's output) of program (prog & 15) = 0 unet / 1 vae / 2 guide, chained-step instance (prog >> 4) */
struct dd_engine;
int dd_debug_tensor(struct dd_engine* e, int prog, int idx, int want_grad, float* host_out, int* info4);
int dd_debug_num_tensors(struct dd_engine* e, int prog);
/* the statistics fusions of program prog = 0 unet / 1 vae / 2 guide / 3 vae encoder, fixed by dd_finalize_weights and read-only from
 * then on: writes min(cap, ops) records of four ints, one per op in program order, and returns the op count (< 0: dd_status).
 *   [0] op kind: 0 convolution / linear, 1 GroupNorm, 2 LayerNorm, > 2 anything else
 *   [1] GroupNorm statistics.  Convolution: 1 emits per-channel partials from its epilogue (CF_STATS), 0 a candidate that does not,
 *       -1 no candidate.  GroupNorm: 1 merges its producers' partials, 0 has partial buffers but runs its own pass, -1 has none
 *   [2] LayerNorm row partials.  Linear: column spans it emits (CF_ROWSTATS), 0 a candidate that does not, -1 no candidate.
 *       LayerNorm: spans it reads from the linear in front of it, 0 folded with its own statistics pass, -1 not folded
 *   [3] reserved, 0 */
int dd_debug_fusion_plan(struct dd_engine* e, int prog, int* out, int cap);
/* The plans without a device.  dd_debug_plan_only, before dd_finalize_weights: from then on the engine allocates fake, never
 * dereferenced addresses (still counted by dd_workspace_bytes), uploads and copies nothing, frees nothing in dd_destroy, and every entry
 * point that would launch or copy returns DD_ERR_STATE: dd_finalize_weights builds and plans every program on a machine without a GPU.
 * dd_debug_plan_dump, after dd_finalize_weights (of any engine): the plans of program prog = 0 unet / 1 vae / 2 guide / 3 vae encoder /
 * 4 text / 5 text2 (a program that was not built is empty) as int64 words; writes min(cap, words) and returns the word count (< 0: dd_status).
 *   program: tensors, ops, act_bytes, grad_bytes, scratch_partial, scratch_tmp, scratch_rowpart, tr_max, tr_count
 *   then per tensor (16): off, goff, parent, rows, C, ld, B, H, W, f32, grad, gf32, transient, tr_slot, glo, ghi
 *   then per op (50): kind, x, y, res, raw, q, k, v, x2, cw, nw (index into the engine's convs / norms, -1 none), stride, up, relu,
 *     out_f32, use_table, G, silu, eps (float bits), heads, D, Nq, Nk, cross_slot, causal, act_kind, pv_fp8, q_prescaled, patch, sel_stride,
 *     stats_off, fused, x_acc, res_acc, x2_acc, res_alias, part, part_off, part_ld, producers (count), producers (FNV-1a hash), gn_fused,
 *     ln_fold, x_fwd, ln_stats_off, rowstat_from, rowstat_emit, rowstat_ld, row_spans, flops (double bits)
 * prog = 6, the engine: total_bytes, partial_cap, tmp_cap, packed buffers, then the size of every packed weight buffer in order */
int dd_debug_plan_only(struct dd_engine* e);
int dd_debug_plan_dump(struct dd_engine* e, int prog, int64_t* out, int cap);
/* parity-test hook: evaluate the guide network of every later guided forward AT these images (DEVICE fp32 [count][B,3,8L,8L], the
 * decoder's output range, caller-owned; chained guided step k reads image min(k, count-1)) instead of the decoder's own output;
 * gradients still flow through the decoder.  The input-gradient of the ReLU / max-pool guide is piecewise constant in the image, so
 * two implementations of torch.autograd.grad(E, ...) (generate_data.py:721, :761) can only be compared at the same image.
 * NULL / count 0 switches it off.  dd_debug_set_image = count 1. */
int dd_debug_set_images(struct dd_engine* e, const float* images, int count);
int dd_debug_set_image(struct dd_engine* e, const float* image);

#ifdef __cplusplus
}
#endif
#endif
