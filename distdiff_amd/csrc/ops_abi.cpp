// extern "C" op-level entry points (include/distdiff_hip_ops.h): thin forwards to the launchers.
#include "kernels.h"
#include "../../include/distdiff_hip_ops.h"

#define S(x) ((hipStream_t)(x))
extern "C" {
int dd_op_conv_gemm(const ConvGemmParams* p, size_t cap, void* st) {
  // Stream-asynchronous like every other launcher (no host round trip: graph-capturable, and back-to-back launches stay back to back).
  // Contract: a one-tap, stride-1, same-size launch is a 1x1 / linear layer and takes the persistent kernels' pointwise path, which
  // does not read the tap table -- it IS the centre tap, what every packer emits for such layers.  The host side that owns the table
  // validates it when the weights are packed (distdiff_amd/ops.py: PackedConv.taptab_host), not here per launch.
  return (int)launch_conv_gemm(*p, cap, S(st));
}
int dd_op_conv_gemm_kind(const ConvGemmParams* p, size_t cap) {
  if (!p) return -1;                                    // DD_ERR_ARG
  return conv_gemm_kind(*p, cap);
}
int dd_op_conv_gemm_plan(const ConvGemmParams* p, size_t cap, int* out4) {
  if (!p) return -1;                                    // DD_ERR_ARG
  return conv_gemm_plan_query(*p, cap, out4);
}
int dd_op_conv_halo_plan(const ConvGemmParams* p, size_t cap, int* out12) {
  if (!p || !out12) return -1;                          // DD_ERR_ARG
  return conv_halo_plan_query(*p, cap, out12);
}
int dd_op_conv_gemm_check(const ConvGemmParams* p, void* st) {
  // The synchronous companion for ABI users who want the contract checked against the DEVICE table: waits for the stream, reads the
  // tap table back and validates it (entries in range; a one-tap stride-1 same-size launch carries the centre tap).  0 = fine.
  if (!p || !p->taptab || p->ntaps < 1 || p->ntaps > 64) return (int)hipErrorInvalidValue;
  int taps[64];
  hipError_t e = hipStreamSynchronize(S(st));
  if (e == hipSuccess) e = hipMemcpy(taps, p->taptab, sizeof(int) * p->ntaps, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return (int)e;
  for (int t = 0; t < p->ntaps; ++t) {
    const int dy = ((taps[t] >> 6) & 63) - 32, dx = (taps[t] & 63) - 32;
    if ((taps[t] >> 12) != 0 || dy < -31 || dy > 31 || dx < -31 || dx > 31) return (int)hipErrorInvalidValue;
  }
  if (p->ntaps == 1 && p->stride == 1 && !p->shift && p->H == p->Ho && p->W == p->Wo && taps[0] != ((32 << 6) | 32)) return (int)hipErrorInvalidValue;
  return 0;
}
int dd_op_groupnorm_fwd(const GroupNormParams* p, void* st) { return (int)launch_groupnorm_fwd(*p, S(st)); }
int dd_op_groupnorm_bwd(const GroupNormParams* p, void* st) { return (int)launch_groupnorm_bwd(*p, S(st)); }
size_t dd_op_groupnorm_scratch_bytes(int B, int G) { return groupnorm_scratch_bytes(B, G); }
int dd_op_layernorm_fwd(const LayerNormParams* p, void* st) { return (int)launch_layernorm_fwd(*p, S(st)); }
int dd_op_layernorm_bwd(const LayerNormParams* p, void* st) { return (int)launch_layernorm_bwd(*p, S(st)); }
int dd_op_attention_fwd(const AttnParams* p, void* st) { return (int)launch_attention_fwd(*p, S(st)); }
int dd_op_attention_bwd(const AttnParams* p, void* st) { return (int)launch_attention_bwd(*p, S(st)); }
int dd_op_attention(const AttnParams* p, void* ws, size_t ws_bytes, const int* tap1x1, float* partial, size_t cap, int bwd, void* st) {
  return (int)launch_attention(*p, AttnScratch{ws, ws_bytes, tap1x1, partial, cap}, bwd != 0, S(st));
}
int dd_op_attention_plan(const AttnParams* p, size_t ws_bytes, int bwd, int* out) {
  if (!p || !out) return -1;                            // DD_ERR_ARG
  return attention_plan_query(*p, ws_bytes, bwd != 0, out);
}
size_t dd_op_attention_scratch_bytes(int B, int heads, int Nq, int Nk, int D, int causal, int cross, int want_grad) {
  return attention_scratch_bytes(B, heads, Nq, Nk, D, causal != 0, cross != 0, want_grad != 0);
}
size_t dd_op_attention_gemm_workspace(int Nq, int Nk, int D, int bwd) { return attention_gemm_workspace(Nq, Nk, D, bwd); }
int dd_op_attention_gemm_fwd(const AttnParams* p, void* ws, size_t ws_bytes, const int* tap1x1, float* partial, size_t cap, void* st) {
  return (int)launch_attention_gemm_fwd(*p, ws, ws_bytes, tap1x1, partial, cap, S(st));
}
int dd_op_attention_gemm_bwd(const AttnParams* p, void* ws, size_t ws_bytes, const int* tap1x1, float* partial, size_t cap, void* st) {
  return (int)launch_attention_gemm_bwd(*p, ws, ws_bytes, tap1x1, partial, cap, S(st));
}

int dd_op_conv_f32(const ConvF32Params* p, void* st) { return (int)launch_conv_f32(*p, S(st)); }
int dd_pack_conv_weight_f32(const float* w, int Cout, int Cin, int KH, int KW, int pad, int mode, int groups, float* wp, int* taptab,
                            int* out4) {
  const PackedConv s = pack_conv_shape_f32(Cout, Cin, KH, KW, mode, groups);
  if (out4) { out4[0] = s.N; out4[1] = s.K; out4[2] = s.cin; out4[3] = s.ntaps; }
  if (wp) pack_conv_weight_f32(w, Cout, Cin, KH, KW, pad, mode, groups, wp, taptab);
  return 0;
}
int dd_pack_conv_weight(const float* w, int Cout, int Cin, int KH, int KW, int pad, int mode, int geglu, uint16_t* wp,
                        int* taptab, int* out4) {
  const PackedConv s = pack_conv_shape(Cout, Cin, KH, KW, mode);
  if (out4) { out4[0] = s.N; out4[1] = s.K; out4[2] = s.cin; out4[3] = s.ntaps; }
  if (wp) pack_conv_weight(w, Cout, Cin, KH, KW, pad, mode, geglu, wp, taptab);
  return 0;
}
int dd_op_nchw_f32_to_nhwc_bf16(const float* src, uint16_t* dst, int B, int C, int H, int W, int Cpad, int ld, int dup,
                                float scale, void* st) {
  return (int)launch_nchw_f32_to_nhwc_bf16(src, dst, B, C, H, W, Cpad, ld, dup, scale, S(st));
}
int dd_op_nhwc_to_nchw_f32(const void* src, int src_f32, float* dst, int B, int C, int H, int W, int ld, float scale, float shift,
                           int clamp, float lo, float hi, void* st) {
  return (int)launch_nhwc_to_nchw_f32(src, src_f32, dst, B, C, H, W, ld, scale, shift, clamp, lo, hi, S(st));
}
// the sampler-step ops: each fills one StepParams (kernels.h lists the modes) for one of the two launchers
static StepParams step_params(const float* m2, int ld, int B, int C, int HW, const float* coef, const float* lin, int prediction_type,
                              float guidance_rescale, const float* stats, float* part) {
  StepParams p{};
  p.m2 = m2; p.ld = ld; p.B = B; p.C = C; p.HW = HW; p.coef = coef; p.lin = lin; p.prediction_type = prediction_type;
  p.phi = guidance_rescale; p.stats = const_cast<float*>(stats); p.part = part;
  return p;
}
// the five coefficient ops on sampler_step_row: a row refused in front of the arithmetic leaves `out` untouched, a row a stochastic rule
// found not finite is written and refused
static int step_row_op(const StepRule& r, double a, double a_prev, float* out, int count) {
  StepRow row;
  if (!out) return -1;
  const int rc = sampler_step_row(r, 0, 0, 0.0, a, a_prev, &row);
  if (rc == -1) return -1;
  for (int k = 0; k < count; ++k) out[k] = k < 4 ? row.lin[k] : row.sigma;
  return rc ? -1 : 0;
}
int dd_op_cfg_ddim(const float* eps2, int ld, const float* z, float* z_prev, float* x0, int B, int C, int HW, const float* coef,
                   void* st) {
  return dd_op_sampler_step(eps2, ld, z, z_prev, x0, B, C, HW, coef, nullptr, 0, 0.f, nullptr, nullptr, st);
}
int dd_op_cfg_ddim_bwd(const float* g_x0, const float* g_zprev, uint16_t* g_eps2, int ld, float* g_z, int B, int C, int HW,
                       const float* coef, void* st) {
  return dd_op_sampler_step_bwd(g_x0, g_zprev, g_eps2, ld, g_z, B, C, HW, coef, nullptr, 0, 0.f, nullptr, nullptr, nullptr, st);
}
int dd_op_step_coefs(int prediction_type, double a, double a_prev, float* out4) {
  return step_row_op({prediction_type, 0, 0.0}, a, a_prev, out4, 4);
}
size_t dd_op_sampler_step_scratch_floats(int B, int HW) { return sampler_step_scratch_floats(B, HW); }
int dd_op_sampler_step(const float* m2, int ld, const float* z, float* z_prev, float* x0, int B, int C, int HW, const float* coef,
                       const float* lin, int prediction_type, float guidance_rescale, float* stats, float* part, void* st) {
  return dd_op_sampler_step_2m(m2, ld, z, nullptr, 0.f, z_prev, x0, B, C, HW, coef, lin, prediction_type, guidance_rescale, stats, part, st);
}
int dd_op_sampler_step_bwd(const float* g_x0, const float* g_zprev, uint16_t* g_m2, int ld, float* g_z, int B, int C, int HW,
                           const float* coef, const float* lin, int prediction_type, float guidance_rescale, const float* m2,
                           const float* stats, float* part, void* st) {
  return (int)launch_sampler_step_bwd(step_params(m2, ld, B, C, HW, coef, lin, prediction_type, guidance_rescale, stats, part), g_x0, g_zprev,
                                      g_m2, g_z, S(st));
}
// c does not depend on the prediction type: it is asked of the v-prediction rule, which refuses no (a, a')
float dd_op_step_coef_2m(int step_index, int n_steps, double a_before, double a, double a_prev) {
  StepRow row;
  sampler_step_row({1, 0, 0.0}, step_index, n_steps, a_before, a, a_prev, &row);
  return row.c2m;
}
int dd_op_sampler_step_2m(const float* m2, int ld, const float* z, const float* x0_prev, float c2m, float* z_prev, float* x0, int B, int C,
                          int HW, const float* coef, const float* lin, int prediction_type, float guidance_rescale, float* stats,
                          float* part, void* st) {
  return dd_op_sampler_step_2m_n(m2, ld, z, x0_prev, c2m, nullptr, 0.f, 0, 0, nullptr, z_prev, x0, B, C, HW, coef, lin, prediction_type,
                                 guidance_rescale, stats, part, st);
}
int dd_op_step_coefs_eta(int prediction_type, double a, double a_prev, double eta, float* out5) {
  return step_row_op({prediction_type, 1, eta}, a, a_prev, out5, 5);
}
int dd_op_sampler_step_n(const float* m2, int ld, const float* z, const float* noise, float sigma, uint64_t seed, int rng_stream,
                         const uint64_t* unit_ids, float* z_prev, float* x0, int B, int C, int HW, const float* coef, const float* lin,
                         int prediction_type, float guidance_rescale, float* stats, float* part, void* st) {
  return dd_op_sampler_step_2m_n(m2, ld, z, nullptr, 0.f, noise, sigma, seed, rng_stream, unit_ids, z_prev, x0, B, C, HW, coef, lin,
                                 prediction_type, guidance_rescale, stats, part, st);
}
int dd_op_step_coefs_sde(int prediction_type, double a, double a_prev, double sde_eta, float* out5) {
  return step_row_op({prediction_type, 2, sde_eta}, a, a_prev, out5, 5);
}
int dd_op_step_coef_2m_sde(int step_index, int n_steps, double a_before, double a, double a_prev, double sde_eta, float* out) {
  StepRow row;
  if (!out || sampler_step_row({1, 2, sde_eta}, step_index, n_steps, a_before, a, a_prev, &row) == -1) return -1;
  *out = row.c2m;
  return 0;
}
int dd_op_sampler_step_2m_n(const float* m2, int ld, const float* z, const float* x0_prev, float c2m, const float* noise, float sigma,
                            uint64_t seed, int rng_stream, const uint64_t* unit_ids, float* z_prev, float* x0, int B, int C, int HW,
                            const float* coef, const float* lin, int prediction_type, float guidance_rescale, float* stats, float* part,
                            void* st) {
  // the general forward op, which the other three call: the optional history (x0_prev, c2m) and the optional noise (the tensor, or seed /
  // stream / unit_ids for the generated form; with neither, sigma stays 0 and the launch is launch_sampler_step's deterministic one)
  StepParams p = step_params(m2, ld, B, C, HW, coef, lin, prediction_type, guidance_rescale, stats, part);
  p.z = z; p.x0_prev = x0_prev; p.c2m = c2m; p.z_prev = z_prev; p.x0 = x0;
  if (noise || unit_ids) { p.noise = noise; p.sigma = sigma; p.rng_seed = seed; p.rng_stream = rng_stream; }
  return (int)launch_sampler_step_units(p, unit_ids, S(st));
}
// the CFG-free step (StepParams::halves = 1): m1 is the conditional output alone, every optional input of dd_op_sampler_step_2m_n, no rescale
int dd_op_sampler_step1(const float* m1, int ld, const float* z, const float* x0_prev, float c2m, const float* noise, float sigma,
                        uint64_t seed, int rng_stream, const uint64_t* unit_ids, float* z_prev, float* x0, int B, int C, int HW,
                        const float* coef, const float* lin, int prediction_type, void* st) {
  StepParams p = step_params(m1, ld, B, C, HW, coef, lin, prediction_type, 0.f, nullptr, nullptr);
  p.halves = 1;
  p.z = z; p.x0_prev = x0_prev; p.c2m = c2m; p.z_prev = z_prev; p.x0 = x0;
  if (noise || unit_ids) { p.noise = noise; p.sigma = sigma; p.rng_seed = seed; p.rng_stream = rng_stream; }
  return (int)launch_sampler_step_units(p, unit_ids, S(st));
}
int dd_op_sampler_step1_bwd(const float* g_x0, const float* g_zprev, uint16_t* g_m1, int ld, float* g_z, int B, int C, int HW,
                            const float* coef, const float* lin, int prediction_type, void* st) {
  StepParams p = step_params(nullptr, ld, B, C, HW, coef, lin, prediction_type, 0.f, nullptr, nullptr);
  p.halves = 1;
  return (int)launch_sampler_step_bwd(p, g_x0, g_zprev, g_m1, g_z, S(st));
}
int dd_op_sumpool2x2(const uint16_t* src, int src_ld, uint16_t* dst, int dst_ld, int B, int H, int W, int C, int acc, void* st) {
  return (int)launch_sumpool2x2(src, src_ld, dst, dst_ld, B, H, W, C, acc, S(st));
}
int dd_op_geglu_bwd(const uint16_t* raw, int ld_raw, const uint16_t* dout, int ld_dout, uint16_t* draw, int ld_draw, int M, int F,
                    void* st) {
  return (int)launch_geglu_bwd(raw, ld_raw, dout, ld_dout, draw, ld_draw, M, F, S(st));
}
int dd_op_maxpool3x3s2(const uint16_t* x, uint16_t* y, int B, int H, int W, int C, void* st) {
  return (int)launch_maxpool3x3s2(x, y, B, H, W, C, S(st));
}
int dd_op_maxpool3x3s2_bwd(const uint16_t* x, const uint16_t* dy, uint16_t* dx, int B, int H, int W, int C, void* st) {
  return (int)launch_maxpool3x3s2_bwd(x, dy, dx, B, H, W, C, S(st));
}
int dd_op_bicubic(const uint16_t* src, int ld_s, uint16_t* dst, int ld_d, int B, int Hs, int Ws, int Hd, int Wd, int C, int Cpad,
                  void* st) {
  return (int)launch_bicubic(src, ld_s, dst, ld_d, B, Hs, Ws, Hd, Wd, C, Cpad, S(st));
}
int dd_op_bicubic_bwd(const uint16_t* ddst, int ld_d, uint16_t* dsrc, int ld_s, int B, int Hs, int Ws, int Hd, int Wd, int C,
                      void* st) {
  return (int)launch_bicubic_bwd(ddst, ld_d, dsrc, ld_s, B, Hs, Ws, Hd, Wd, C, S(st));
}
int dd_op_gap(const uint16_t* x, int ld, float* f, int B, int HW, int C, void* st) { return (int)launch_gap(x, ld, f, B, HW, C, S(st)); }
int dd_op_energy(const float* f, const float* Pc, const float* Pg, const int* targets, int B, int D, int K, float gs, float ls,
                 int use_c, int use_g, int normalize, float weight, float* score_out, float* gf, void* st) {
  return (int)launch_energy(f, Pc, Pg, targets, B, D, K, gs, ls, use_c, use_g, normalize, weight, nullptr, score_out, nullptr, gf, S(st));
}
int dd_op_transform_update(const float* z, const float* g, const float* e, const float* b, float* z_out, int BC, int HW, float rho,
                           float c, void* st) {
  return (int)launch_transform_update(z, g, e, b, z_out, BC, HW, rho, c, S(st));
}
int dd_op_affine(const float* z, const float* e, const float* b, float* out, int BC, int HW, void* st) {
  return (int)launch_affine(z, e, b, out, BC, HW, S(st));
}

// the side kernels of the reverse programs
int dd_op_mask_bf16(const uint16_t* dy, int ldd, const uint16_t* mask, int ldm, uint16_t* y, int ldy, int M, int C, void* st) {
  return (int)launch_mask_bf16(dy, ldd, mask, ldm, y, ldy, M, C, S(st));
}
int dd_op_add_bf16(const uint16_t* a, int lda, const uint16_t* b, int ldb, uint16_t* y, int ldy, int M, int C, void* st) {
  return (int)launch_add_bf16(a, lda, b, ldb, y, ldy, M, C, S(st));
}
int dd_op_copy_bf16(const uint16_t* a, int lda, uint16_t* y, int ldy, int M, int C, void* st) { return (int)launch_copy_bf16(a, lda, y, ldy, M, C, S(st)); }
int dd_op_dup_bwd(const uint16_t* gin, int ld, float* g_z, int B, int C, int HW, int accumulate, int halves, void* st) {
  return (int)launch_dup_bwd(gin, ld, g_z, B, C, HW, accumulate, halves, S(st));
}
int dd_op_gap_bwd(const float* gf, uint16_t* dx, int ld, int B, int HW, int C, const uint16_t* mask, int mask_ld, void* st) {
  return (int)launch_gap_bwd(gf, dx, ld, B, HW, C, mask, mask_ld, S(st));
}
int dd_op_act_bf16(const uint16_t* x, int ldx, uint16_t* y, int ldy, int M, int C, int kind, void* st) {
  return (int)launch_act_bf16(x, ldx, y, ldy, M, C, kind, S(st));
}
int dd_op_act_bwd_bf16(const uint16_t* x, int ldx, const uint16_t* dy, int ldd, uint16_t* dx, int ldo, int M, int C, int kind, int accumulate,
                       void* st) {
  return (int)launch_act_bwd_bf16(x, ldx, dy, ldd, dx, ldo, M, C, kind, accumulate, S(st));
}
int dd_op_patchify(const float* img, int ld, uint16_t* out, int B, int Sz, int p, int C, void* st) { return (int)launch_patchify(img, ld, out, B, Sz, p, C, S(st)); }
int dd_op_patchify_bwd(const uint16_t* gout, float* gimg, int ld, int B, int Sz, int p, int C, void* st) {
  return (int)launch_patchify_bwd(gout, gimg, ld, B, Sz, p, C, S(st));
}
int dd_op_vit_embed(const uint16_t* patches, int ldp, const float* cls, const float* pos, uint16_t* out, int ldo, int B, int np, int W, void* st) {
  return (int)launch_vit_embed(patches, ldp, cls, pos, out, ldo, B, np, W, S(st));
}
int dd_op_vit_embed_bwd(const uint16_t* gout, int ldo, uint16_t* gp, int ldp, int B, int np, int W, void* st) {
  return (int)launch_vit_embed_bwd(gout, ldo, gp, ldp, B, np, W, S(st));
}
int dd_op_select_rows(const uint16_t* x, int ldx, uint16_t* y, int ldy, int B, int stride, int C, void* st) {
  return (int)launch_select_rows(x, ldx, y, ldy, B, stride, C, S(st));
}
int dd_op_select_rows_bwd(const uint16_t* dy, int ldy, uint16_t* dx, int ldx, int B, int stride, int C, int accumulate, void* st) {
  return (int)launch_select_rows_bwd(dy, ldy, dx, ldx, B, stride, C, accumulate, S(st));
}
int dd_op_sub_scaled(const float* a, const float* g, float* out, size_t n, float rho, void* st) { return (int)launch_sub_scaled(a, g, out, n, rho, S(st)); }
int dd_op_energy_weighted(const float* f, const float* Pc, const float* Pg, const int* targets, int B, int D, int K, float gs, float ls,
                          int use_c, int use_g, int normalize, float weight, const float* sample_w, float* score_out, float* image_scores,
                          float* gf, void* st) {
  return (int)launch_energy(f, Pc, Pg, targets, B, D, K, gs, ls, use_c, use_g, normalize, weight, sample_w, score_out, image_scores, gf, S(st));
}
int dd_op_mask_f32(const float* dy, int ldd, const float* mask, int ldm, float* y, int ldy, int M, int C, float hi, void* st) {
  return (int)launch_mask_f32(dy, ldd, mask, ldm, y, ldy, M, C, hi, S(st));
}
int dd_op_add_f32(const float* a, int lda, const float* b, int ldb, float* y, int ldy, int M, int C, void* st) {
  return (int)launch_add_f32(a, lda, b, ldb, y, ldy, M, C, S(st));
}
int dd_op_copy_f32(const float* a, int lda, float* y, int ldy, int M, int C, void* st) { return (int)launch_copy_f32(a, lda, y, ldy, M, C, S(st)); }
int dd_op_maxpool3x3s2_f32(const float* x, float* y, int B, int H, int W, int C, void* st) { return (int)launch_maxpool3x3s2_f32(x, y, B, H, W, C, S(st)); }
int dd_op_maxpool3x3s2_bwd_f32(const float* x, const float* dy, float* dx, int B, int H, int W, int C, void* st) {
  return (int)launch_maxpool3x3s2_bwd_f32(x, dy, dx, B, H, W, C, S(st));
}
int dd_op_bicubic_f32(const float* src, int ld_s, float* dst, int ld_d, int B, int Hs, int Ws, int Hd, int Wd, int C, int Cpad, void* st) {
  return (int)launch_bicubic_f32(src, ld_s, dst, ld_d, B, Hs, Ws, Hd, Wd, C, Cpad, S(st));
}
int dd_op_bicubic_bwd_f32(const float* ddst, int ld_d, void* dsrc, int dsrc_bf16, int ld_s, int B, int Hs, int Ws, int Hd, int Wd, int C,
                          void* st) {
  return (int)launch_bicubic_bwd_f32(ddst, ld_d, dsrc, dsrc_bf16, ld_s, B, Hs, Ws, Hd, Wd, C, S(st));
}
int dd_op_gap_f32(const float* x, int ld, float* f, int* argmax, int B, int HW, int C, int use_max, void* st) {
  return (int)launch_gap_f32(x, ld, f, argmax, B, HW, C, use_max, S(st));
}
int dd_op_gap_bwd_f32(const float* gf, float* dx, int ld, int B, int HW, int C, const int* argmax, void* st) {
  return (int)launch_gap_bwd_f32(gf, dx, ld, B, HW, C, argmax, S(st));
}
int dd_op_nchw_to_nhwc_f32(const float* src, float* dst, int B, int C, int H, int W, int Cpad, int ld, void* st) {
  return (int)launch_nchw_to_nhwc_f32(src, dst, B, C, H, W, Cpad, ld, S(st));
}
}
