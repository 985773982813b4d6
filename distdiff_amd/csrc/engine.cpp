// The expansion engine: a static op-graph executor for the SD-1.x UNet, the AutoencoderKL decoder and the
// ResNet-50 guide, with a hand-derived reverse program (input-gradients only, no autograd) composed from
// per-op VJPs, plus the guided DDIM sampler drivers behind the C ABI of include/distdiff_hip.h.
//
// Reference functions replaced: generate_data.py:109-121 (denoise_one_step), :687-732 (transform_guidance),
// :735-767 (direct_guidance), :1161-1228 (loop + decode); diffusers / timm module forwards as listed in
// SURVEY.md section 8a. Activations are NHWC bf16 matrices; every forward op stashes what its VJP needs
// (288 GB HBM makes a full stash viable), the reverse program is built once at finalize time.
#include "engine_internal.h"

namespace {
// ---- sampler drivers ----
// execution context of program P on the activation slab `act`; of prog[p] on its slab of instance k
Ctx make_ctx(dd_engine* E, const Program& P, char* act, hipStream_t s) {
  Ctx c; c.act = act; c.grad = E->grad_slab; c.tr = E->tr_slab; c.tr_stride = P.tr_max; c.scratch_partial = E->scratch_partial; c.partial_cap = E->partial_cap;
  c.scratch_tmp = E->scratch_tmp; c.tmp_cap = E->tmp_cap; c.tap1x1 = E->tap1x1; c.gn_scratch = E->gn_scratch; c.rowpart = E->rowpart; c.s = s; c.cross_kv = &E->cross_kv; c.flops = &E->flops; c.prof = &E->prof;
  return c;
}
Ctx make_ctx(dd_engine* E, int p, int k, hipStream_t s) { return make_ctx(E, E->prog[p], E->inst[k].act[p], s); }

void check_batch(dd_engine* E, int B, bool need_grad = false) {
  if (B != E->cfg.max_batch) throw std::runtime_error("this engine was built for batch " + std::to_string(E->cfg.max_batch) +
                                                      " (static shapes); got B=" + std::to_string(B));
  if (!E->finalized) throw std::runtime_error("dd_finalize_weights has not been called");
  if (need_grad && !E->cfg.enable_grad) throw std::runtime_error("engine created with enable_grad=0");
}

// Cotangent scale of the fp16 build (common.h: CotScale).  cot_normalise computes {s, 1 / s} from the fp32 cotangent(s) in front of a
// reverse program and returns the device pointer to s for the entry kernel; cot_inv(that) is what the exit kernel takes.  The bf16
// build launches nothing and hands null to both.
#ifdef DD_ACT_F16
const float* cot_normalise(dd_engine* E, const float* g, size_t rows, int C, int ld, hipStream_t s, const float* g2 = nullptr) {
  HIPCHK(launch_cot_scale(g, rows, C, ld, g2, rows, C, ld, E->cot_part, E->cot_scale, s));
  return E->cot_scale;
}
void cot_mul(float* x, size_t rows, int C, int ld, const float* mul, hipStream_t s) { HIPCHK(launch_cot_mul(x, rows, C, ld, mul, s)); }
#else
inline const float* cot_normalise(dd_engine*, const float*, size_t, int, int, hipStream_t, const float* = nullptr) { return nullptr; }
inline void cot_mul(float*, size_t, int, int, const float*, hipStream_t) {}
#endif
inline const float* cot_inv(const float* cs) { return cs ? cs + 1 : nullptr; }

// UNet forward on instance k: z fp32 NCHW -> eps2 fp32 NHWC [halves*B*HW, ld] inside the slab (a CFG-free engine: the conditional output alone)
void unet_fwd(dd_engine* E, int k, const float* z, int step_index, hipStream_t s, bool stash = true) {
  const dd_config& c = E->cfg;
  Ctx ctx = make_ctx(E, dd_engine::UNET, k, s);
  ctx.step_index = step_index;
  ctx.stash = stash;
  if (c.unet_add_time_dim > 0) {
    if (!E->added_cond_set) throw std::runtime_error("this UNet has text_time additional conditioning: call dd_set_added_cond first");
    ctx.img_bias = 2 * c.max_batch;
  }
  const Tn& in = E->unet.t[E->unet_in];
  HIPCHK(launch_nchw_f32_to_nhwc_bf16(z, act_ptr(ctx, in), c.max_batch, c.unet_in_channels, c.latent_size, c.latent_size, in.ld, in.ld,
                                      in.B == 2 * c.max_batch ? 1 : 0, 1.f, s));
  run_fwd(E->unet, ctx);
}

void vae_fwd(dd_engine* E, int k, const float* x0, hipStream_t s) {
  const dd_config& c = E->cfg;
  Ctx ctx = make_ctx(E, dd_engine::VAE, k, s);
  const Tn& in = E->vae.t[E->vae_in];
  HIPCHK(launch_nchw_f32_to_nhwc_bf16(x0, act_ptr(ctx, in), c.max_batch, c.vae_latent_channels, c.latent_size, c.latent_size, in.ld,
                                      in.ld, 0, 1.f / c.vae_scaling_factor, s));
  run_fwd(E->vae, ctx);
}

// features of a finished guide forward -> feats [B, D] fp32: global average pool of the last feature map (ResNets, model_utils.py:31-33)
// or the projected class token (ViT)
void guide_features_out(dd_engine* E, const Ctx& gc, float* feats, hipStream_t s, int use_max = 0) {
  const dd_config& c = E->cfg;
  const Tn& f = E->guide.t[E->guide_feat];
  if (c.guide_kind == 1) HIPCHK(hipMemcpy2DAsync(feats, (size_t)f.C * 4, act_f32(gc, f), (size_t)f.ld * 4, (size_t)f.C * 4, f.rows, hipMemcpyDeviceToDevice, s));
  else HIPCHK(launch_gap_f32(act_f32(gc, f), f.ld, feats, nullptr, c.max_batch, f.H * f.W, f.C, use_max, s));
}
// cotangent of the features [B, D] fp32 -> gradient of the guide's output tensor (reverse of guide_features_out).  Returns the
// cotangent scale the 16-bit ViT program was entered with (null: the fp32 guides, the bf16 build)
const float* guide_features_grad_in(dd_engine* E, const Ctx& gc, const float* gfeat, hipStream_t s) {
  const dd_config& c = E->cfg;
  const Tn& f = E->guide.t[E->guide_feat];
  if (c.guide_kind == 1) {
    if (f.ld != f.C) throw std::runtime_error("ViT guide: feature dim must be a multiple of 8");
    const float* cs = cot_normalise(E, gfeat, f.rows, f.C, f.C, s);
    HIPCHK(launch_f32_to_bf16(gfeat, grad_ptr(gc, f), (size_t)f.rows * f.C, s, cs));
    return cs;
  }
  HIPCHK(launch_gap_bwd_f32(gfeat, grad_f32(gc, f), f.ld, c.max_batch, f.H * f.W, f.C, nullptr, s));
  return nullptr;
}

// guide forward from the decoded image of instance k (bicubic -> guide network -> features) -> feat [B, D]
void guide_fwd_from_image(dd_engine* E, int k, hipStream_t s) {
  const dd_config& c = E->cfg;
  Ctx gc = make_ctx(E, dd_engine::GUIDE, k, s);
  Ctx vc = make_ctx(E, dd_engine::VAE, k, s);
  const Tn& img = E->vae.t[E->vae_out];
  const Tn& gin = E->guide.t[E->guide_in];
  // the decoder's conv_out stores the image in fp32: image, bicubic resize and the whole guide stay fp32
  if (E->image_override) {  // parity tests: the guide (its ReLU / max-pool masks) is evaluated AT the given image, gradients flow as usual
    const size_t per = (size_t)c.max_batch * c.vae_out_channels * img.H * img.W;
    const float* src = E->image_override + per * std::min(k, E->image_override_count - 1);
    HIPCHK(launch_nchw_to_nhwc_f32(src, act_f32(vc, img), c.max_batch, c.vae_out_channels, img.H, img.W, img.ld, img.ld, s));
  }
  HIPCHK(launch_bicubic_f32(act_f32(vc, img), img.ld, act_f32(gc, gin), gin.ld, c.max_batch, img.H, img.W, gin.H, gin.W, 3, gin.ld, s));
  run_fwd(E->guide, gc);
  guide_features_out(E, gc, E->inst[k].feat, s);
}

// reverse of guide_fwd_from_image + vae_fwd: gfeat -> g_x0 (fp32 NCHW)
void guide_vae_bwd(dd_engine* E, int k, float* g_x0, hipStream_t s) {
  const dd_config& c = E->cfg;
  Ctx gc = make_ctx(E, dd_engine::GUIDE, k, s);
  Ctx vc = make_ctx(E, dd_engine::VAE, k, s);
  // GAP^T; the ReLU mask of the last bottleneck is applied by that conv op's backward
  const float* gcs = guide_features_grad_in(E, gc, E->inst[k].gfeat, s);
  run_bwd(E->guide, gc);
  const Tn& gin = E->guide.t[E->guide_in];
  const Tn& img = E->vae.t[E->vae_out];
  // the ViT program's exit is its own patch re-layout into the fp32 image gradient: unscaled in place (fp16 build only)
  if (gcs) cot_mul(grad_f32(gc, gin), gin.rows, 3, gin.ld, cot_inv(gcs), s);
  // the guide (fp32) and VAE (bf16) gradient regions are disjoint parts of the shared gradient slab (see finalize)
  const float* cs = cot_normalise(E, grad_f32(gc, gin), gin.rows, 3, gin.ld, s);
  HIPCHK(launch_bicubic_bwd_f32(grad_f32(gc, gin), gin.ld, grad_ptr(vc, img), 1, img.ld, c.max_batch, img.H, img.W, gin.H, gin.W, 3, s, cs));
  run_bwd(E->vae, vc);
  const Tn& vin = E->vae.t[E->vae_in];
  HIPCHK(launch_nhwc_to_nchw_f32(grad_ptr(vc, vin), 0, g_x0, c.max_batch, c.vae_latent_channels, c.latent_size, c.latent_size, vin.ld,
                                 1.f / c.vae_scaling_factor, 0.f, 0, 0.f, 0.f, s, cot_inv(cs)));
}

// The sampler step on the UNet output of instance k (kernels.h: StepParams lists its modes) on the given rows of the schedule, and its VJP
StepParams step_params(dd_engine* E, int k, int step_index, const Schedule::Rows& rows) {
  const dd_config& c = E->cfg;
  const Tn& out = E->unet.t[E->unet_out];
  StepParams p{};
  p.m2 = (const float*)(E->inst[k].act[dd_engine::UNET] + out.off); p.ld = out.ld;
  p.B = c.max_batch; p.C = c.unet_out_channels; p.HW = c.latent_size * c.latent_size;
  p.coef = rows.coef + (size_t)step_index * 8; p.lin = rows.lin + (size_t)step_index * 4;
  p.prediction_type = E->sp.prediction_type; p.phi = E->sp.guidance_rescale;
  p.stats = E->inst[k].rs_stats; p.part = E->rs_part;
  p.halves = E->halves;
  return p;
}
// the noise of a stochastic step (eta > 0 or sde_eta > 0): the caller's tensor [B,C,L,L], or generated inside the step kernel from (seed, unit id of
// the row, stream 16 + step index) -- what dd_randn_units writes for that stream.  Neither: the deterministic step
struct StepNoise {
  const float* noise = nullptr; const uint64_t* unit_ids = nullptr; uint64_t seed = 0;
  bool on() const { return noise || unit_ids; }
};
const StepNoise DETERMINISTIC;
// x0_prev: x0 of step_index - 1 under DPM-Solver++(2M), or null; x0 may be null
void sampler_step(dd_engine* E, int k, const float* z, int step_index, const float* x0_prev, float* z_prev, float* x0, hipStream_t s,
                  const StepNoise& sn) {
  const Schedule::Rows& rows = E->sched.rows(step_index, sn.on());
  const StepRow& row = rows.row[step_index];
  StepParams p = step_params(E, k, step_index, rows);
  p.z = z; p.z_prev = z_prev; p.x0_prev = x0_prev;
  if (row.sigma != 0.f) {           // the stochastic rows
    p.sigma = row.sigma; p.noise = sn.noise;
    p.rng_seed = sn.seed; p.rng_stream = DD_RNG_STEP_STREAM + step_index;
  }
  // a history comes with solver 1 alone (history_refused): under sde_eta > 0 the stochastic rows carry their own c
  p.c2m = x0_prev ? row.c2m : 0.f;
  // the second-order term needs x0 of this step: a caller that does not ask for it has it written to the instance's own buffer
  const bool second_order = x0_prev && p.c2m != 0.f;
  p.x0 = !x0 && second_order ? E->inst[k].x0 : x0;
  HIPCHK(launch_sampler_step_units(p, sn.unit_ids, s));      // sigma = 0: launch_sampler_step(p)
}
// every backward differentiates the deterministic step
void sampler_step_bwd(dd_engine* E, int k, const Ctx& uc, int step_index, const float* g_x0, const float* g_znext, float* g_z, hipStream_t s) {
  HIPCHK(launch_sampler_step_bwd(step_params(E, k, step_index, E->sched.det), g_x0, g_znext, grad_ptr(uc, E->unet.t[E->unet_out]), g_z, s));
}
// a history is the input of DPM-Solver++(2M) alone: the step-level entry points refuse it under another solver
bool history_refused(dd_engine* E, const float* x0_prev) {
  const bool refused = x0_prev && !E->sched.keeps_history();
  if (refused) E->err = "x0_prev is the history of DPM-Solver++(2M): this schedule was set with solver 0 (DDIM)";
  return refused;
}
// step noise is the input of a schedule set with eta > 0 or sde_eta > 0 alone
bool noise_refused(dd_engine* E, const float* step_noise) {
  const bool refused = step_noise && !E->sched.stochastic();
  if (refused) E->err = "step_noise is the noise of a stochastic DDIM step: this schedule was set with eta = 0";
  return refused;
}

// one guided forward step on instance k: z_in -> (z_next, x0, feat) ; energy accumulates into score, writes gfeat.  x0_prev: the
// history of a DPM-Solver++(2M) step, sn: the noise of a stochastic step (direct guidance); they change z_next alone, which the reverse
// pass does not differentiate there
void guided_forward(dd_engine* E, int k, const float* z_in, int step_index, const int* targets, int normalize, float weight,
                    float* score, hipStream_t s, const float* x0_prev, const StepNoise& sn) {
  const dd_config& c = E->cfg;
  auto& I = E->inst[k];
  unet_fwd(E, k, z_in, step_index, s);
  sampler_step(E, k, z_in, step_index, x0_prev, I.z_next, I.x0, s, sn);
  vae_fwd(E, k, I.x0, s);
  guide_fwd_from_image(E, k, s);
  HIPCHK(launch_energy(I.feat, E->Pc, E->Pg, targets, c.max_batch, E->pD, E->pK, E->sp.gs, E->sp.ls, E->sp.use_global, E->sp.use_local,
                       normalize, weight, E->sample_w_set ? E->sample_w : nullptr, score, E->image_scores, I.gfeat, s));
}

// reverse of guided_forward: given g_znext (may be null) returns g_z (fp32 NCHW) in g_z_out
// (g_znext and g_x0_tmp are the engine's own buffers and are dead after this call: the fp16 build scales them in place)
void guided_backward(dd_engine* E, int k, int step_index, float* g_znext, float* g_z_out, float* g_x0_tmp, hipStream_t s) {
  const dd_config& c = E->cfg;
  const int HW = c.latent_size * c.latent_size;
  guide_vae_bwd(E, k, g_x0_tmp, s);
  Ctx uc = make_ctx(E, dd_engine::UNET, k, s);
  uc.step_index = step_index;
  // The UNet's reverse program is entered through the sampler step's VJP, which also writes the direct part of g_z: the fp16 build
  // scales both of its fp32 inputs, so that g_z_out carries the scale until the UNet's part has been added, and unscales it at the end
  const size_t zrows = (size_t)c.max_batch * c.unet_out_channels;
  const float* cs = cot_normalise(E, g_x0_tmp, zrows, HW, HW, s, g_znext);
  if (cs) {
    cot_mul(g_x0_tmp, zrows, HW, HW, cs, s);
    if (g_znext) cot_mul(g_znext, zrows, HW, HW, cs, s);
  }
  sampler_step_bwd(E, k, uc, step_index, g_x0_tmp, g_znext, g_z_out, s);
  run_bwd(E->unet, uc);
  const Tn& in = E->unet.t[E->unet_in];
  HIPCHK(launch_dup_bwd(grad_ptr(uc, in), in.ld, g_z_out, c.max_batch, c.unet_in_channels, HW, 1, in.B == 2 * c.max_batch ? 2 : 1, s));
  if (cs) cot_mul(g_z_out, (size_t)c.max_batch * c.unet_in_channels, HW, HW, cot_inv(cs), s);
}

void set_config_defaults(dd_config& c) {
  if (c.max_guidance_period < 1) c.max_guidance_period = 1;
  // same-binary A/B from the environment (tools/, bench.py --config sdxl); an engine built with the field set does not need it
  if (!c.unet_attn_fp8 && getenv("DD_ATTN_FP8")) c.unet_attn_fp8 = atoi(getenv("DD_ATTN_FP8")) != 0;
}

}  // namespace

// ==== C ABI ====
// The body of an entry point that launches or copies, its status to rc: an exception becomes DD_ERR_HIP with its message, and an engine
// that only plans (dd_debug_plan_only) refuses with DD_ERR_STATE.  DD_TRY: the same as the rest of the function
#define DD_TRY_RC(E, rc, ...)                                                                                                        \
  if ((E)->plan_only) { (E)->err = "this engine only plans (dd_debug_plan_only): it owns no device memory"; rc = DD_ERR_STATE; }   \
  else try { __VA_ARGS__; rc = DD_OK; }                                                                                            \
  catch (const std::exception& ex) { (E)->err = ex.what(); rc = DD_ERR_HIP; }
#define DD_TRY(E, ...) { int _rc; DD_TRY_RC(E, _rc, __VA_ARGS__) return _rc; }

extern "C" {

int dd_abi_version(void) { return DD_ABI_VERSION; }
#ifdef DD_ACT_F16
int dd_act_dtype(void) { return 1; }
#else
int dd_act_dtype(void) { return 0; }
#endif

int dd_create(const dd_config* cfg, dd_engine** out) {
  if (!cfg || !out) return DD_ERR_ARG;
  if (cfg->abi_version != DD_ABI_VERSION) {
    fprintf(stderr, "dd_create: dd_config.abi_version %d, library built as %d (caller compiled against another include/distdiff_hip.h?)\n",
            cfg->abi_version, DD_ABI_VERSION);
    return DD_ERR_ARG;
  }
  if (cfg->unet_levels > DD_MAX_LEVELS || cfg->vae_levels > DD_MAX_LEVELS || cfg->guide_stages > DD_MAX_LEVELS || cfg->max_batch < 1)
    return DD_ERR_ARG;
#ifdef DD_ACT_F16
  if (cfg->unet_attn_fp8 || getenv("DD_ATTN_FP8")) {
    fprintf(stderr, "dd_create: the fp16 library has no fp8 P.V attention (unet_attn_fp8 / DD_ATTN_FP8)\n");
    return DD_ERR_ARG;
  }
#endif
  dd_engine* e = new dd_engine();      // reads the plan switches (PlanSwitches)
  e->cfg = *cfg;
  set_config_defaults(e->cfg);
  *out = e;
  return DD_OK;
}

void dd_destroy(dd_engine* e) {
  if (!e) return;
  if (!e->plan_only) for (void* p : e->dev_allocs) hipFree(p);
  delete e;
}

const char* dd_last_error(dd_engine* e) { return e ? e->err.c_str() : "null engine"; }

int dd_load_tensor(dd_engine* e, const char* model, const char* key, const float* data, int ndim, const int64_t* shape) {
  if (!e || !model || !key || !data || ndim < 1 || ndim > 4) return DD_ERR_ARG;
  if (e->finalized) { e->err = "dd_load_tensor after dd_finalize_weights"; return DD_ERR_STATE; }
  HostTensor t;
  t.shape.assign(shape, shape + ndim);
  t.data.assign(data, data + t.numel());
  e->raw[std::string(model) + "/" + key] = std::move(t);
  return DD_OK;
}

int dd_declare_tensor(dd_engine* e, const char* model, const char* key, int ndim, const int64_t* shape) {
  if (!e || !model || !key || ndim < 1 || ndim > 4 || !shape) return DD_ERR_ARG;
  if (e->finalized) { e->err = "dd_declare_tensor after dd_finalize_weights"; return DD_ERR_STATE; }
  HostTensor t;
  t.shape.assign(shape, shape + ndim);
  e->raw[std::string(model) + "/" + key] = std::move(t);
  e->declared++;
  return DD_OK;
}

size_t dd_packed_bytes(dd_engine* e) {
  if (!e) return 0;
  size_t n = 0;
  for (auto& p : e->packed) n += rup_sz(p.second, 256);
  return n;
}

// the packed weights as one virtual byte array (each buffer padded to 256 bytes): copy [offset, offset + bytes) to / from `buf`
static int packed_copy(dd_engine* E, char* buf, size_t offset, size_t bytes, bool to_engine, hipStream_t s) {
  DD_TRY(E, {
    if (!E->finalized) throw std::runtime_error("dd_finalize_weights has not been called");
    size_t pos = 0;
    const size_t end = offset + bytes;
    for (auto& p : E->packed) {
      const size_t lo = std::max(pos, offset), hi = std::min(pos + p.second, end);
      if (lo < hi) {
        char* dev = p.first + (lo - pos);
        char* b = buf + (lo - offset);
        HIPCHK(hipMemcpyAsync(to_engine ? dev : b, to_engine ? b : dev, hi - lo, hipMemcpyDeviceToDevice, s));
      }
      pos += rup_sz(p.second, 256);
      if (pos >= end) break;
    }
  });
}
int dd_export_packed(dd_engine* e, void* dst, size_t offset, size_t bytes, void* stream) {
  if (!e || !dst) return DD_ERR_ARG;
  return packed_copy(e, (char*)dst, offset, bytes, false, (hipStream_t)stream);
}
int dd_import_packed(dd_engine* e, const void* src, size_t offset, size_t bytes, void* stream) {
  if (!e || !src) return DD_ERR_ARG;
  return packed_copy(e, (char*)src, offset, bytes, true, (hipStream_t)stream);
}

int dd_finalize_weights(dd_engine* E) {
  if (!E) return DD_ERR_ARG;
  if (E->finalized) { E->err = "already finalized"; return DD_ERR_STATE; }
  if (E->declared && E->declared != (int)E->raw.size()) { E->err = "dd_declare_tensor and dd_load_tensor cannot be mixed"; return DD_ERR_STATE; }
  E->shape_only = E->declared > 0;
  try {      // not DD_TRY: this is what an engine that only plans is for
    const dd_config& c = E->cfg;
    // the sampler step reads the UNet output as one 8-wide fp32 row per pixel (kernels.h: StepParams)
    if (c.unet_out_channels > 8) throw std::runtime_error("unet_out_channels " + std::to_string(c.unet_out_channels) + " > 8: the sampler step takes at most 8");
    build_unet(E);
    build_vae(E);
    if (c.guide_kind == 1) build_guide_vit(E);
    else if (c.guide_kind == 2) build_guide_mbv2(E);
    else build_guide(E);
    const bool have_venc = E->has("vae", "encoder.conv_in.weight");
    const bool have_text = E->has("text", "text_model.embeddings.token_embedding.weight");
    if (have_venc) build_vae_encoder(E);
    const bool have_text2 = E->has("text2", "text_model.embeddings.token_embedding.weight");
    if (have_text2 && !have_text) throw std::runtime_error("a second text tower (text2) needs the first one (text)");
    if (have_text) build_text_encoder(E, 0);
    if (have_text2) build_text_encoder(E, 1);
    // time embedding MLP weights (fp32, setup-time only)
    auto up = [&](const char* key) {
      const HostTensor& t = E->get("unet", key);
      return (float*)E->wupload(t.data.data(), t.numel() * 4);
    };
    E->temb_w1 = up("time_embedding.linear_1.weight"); E->temb_b1 = up("time_embedding.linear_1.bias");
    E->temb_w2 = up("time_embedding.linear_2.weight"); E->temb_b2 = up("time_embedding.linear_2.bias");
    if (c.unet_add_time_dim > 0) {
      E->add_w1 = up("add_embedding.linear_1.weight"); E->add_b1 = up("add_embedding.linear_1.bias");
      E->add_w2 = up("add_embedding.linear_2.weight"); E->add_b2 = up("add_embedding.linear_2.bias");
    }
    E->raw.clear();
    // activation slabs
    const int P = c.enable_grad ? c.max_guidance_period : 1;
    const int B = c.max_batch, L = c.latent_size;
    const size_t zbytes = (size_t)B * std::max(c.unet_in_channels, c.vae_latent_channels) * L * L * 4;
    E->inst.resize(P);
    for (int k = 0; k < P; ++k) {
      auto& I = E->inst[k];
      for (int p = dd_engine::UNET; p <= dd_engine::GUIDE; ++p)
        if (p == dd_engine::UNET || k == 0 || c.enable_grad) I.act[p] = (char*)E->dmalloc(E->prog[p].act_bytes);
      I.z_in = (float*)E->dmalloc(zbytes); I.z_next = (float*)E->dmalloc(zbytes); I.x0 = (float*)E->dmalloc(zbytes);
      I.feat = (float*)E->dmalloc((size_t)B * guide_feat_dim(c) * 4);
      I.gfeat = (float*)E->dmalloc((size_t)B * guide_feat_dim(c) * 4);
      I.rs_stats = (float*)E->dmalloc((size_t)B * 8 * 4);
    }
    // the CFG-rescale backward re-reads the UNet's forward output of its step: it must live in the instance slab
    if (E->unet.t[E->unet_out].transient) throw std::runtime_error("the UNet output is a transient tensor");
    E->rs_part = (float*)E->dmalloc(sampler_step_scratch_floats(B, L * L) * 4);
#ifdef DD_ACT_F16
    if (c.enable_grad) {
      E->cot_part = (float*)E->dmalloc(cot_scale_scratch_floats() * 4);
      E->cot_scale = (float*)E->dmalloc(2 * 4);
    }
#endif
    // what the programs share is sized for the largest of them
    size_t tr_max = 256;
    E->partial_cap = (size_t)1 << 20; E->tmp_cap = 256;
    for (const Program& P : E->prog) {
      tr_max = std::max(tr_max, P.tr_max); E->partial_cap = std::max(E->partial_cap, P.scratch_partial);
      E->tmp_cap = std::max(E->tmp_cap, P.scratch_tmp);
    }
    E->tr_slab = (char*)E->dmalloc(2 * tr_max);
    if (c.enable_grad) {
      // UNet gradients alone; VAE and guide gradients live side by side (bicubic^T bridges them)
      const size_t g = std::max(E->unet.grad_bytes, E->vae.grad_bytes + E->guide.grad_bytes);
      E->grad_slab = (char*)E->dmalloc(g);
      for (auto& t : E->guide.t) t.goff += E->vae.grad_bytes;
    }
    // encoder programs run before the loop: the image encoder borrows the decoder slab of instance 0 when it fits
    if (have_venc) E->venc_slab = E->venc.act_bytes <= E->vae.act_bytes ? E->inst[0].act[dd_engine::VAE] : (char*)E->dmalloc(E->venc.act_bytes);
    const bool have_tower[2] = {have_text, have_text2};
    for (int w = 0; w < 2; ++w)
      if (have_tower[w]) E->tower[w].slab = (char*)E->dmalloc(E->prog[dd_engine::TEXT + w].act_bytes);
    E->scratch_partial = (char*)E->dmalloc(E->partial_cap, false);
    {
      const int tap = (32 << 6) | 32;
      E->tap1x1 = (int*)E->dmalloc(sizeof(int), false);
      if (!E->plan_only) HIPCHK(hipMemcpy(E->tap1x1, &tap, sizeof(int), hipMemcpyHostToDevice));
    }
    E->scratch_tmp = (char*)E->dmalloc(E->tmp_cap);
    const int maxG = std::max(c.unet_groups, c.vae_groups);
    E->gn_scratch = (float*)E->dmalloc(groupnorm_scratch_bytes(E->halves * B, maxG), false);
    E->rowpart = (float*)E->dmalloc(std::max(E->unet.scratch_rowpart, (size_t)256), false);
    for (auto& f : E->f32_tmp) f = (float*)E->dmalloc(zbytes);
    E->img_tmp = (float*)E->dmalloc((size_t)B * 3 * 64 * L * L * 4);
    E->score_tmp = (float*)E->dmalloc(256);
    E->sample_w = (float*)E->dmalloc((size_t)B * 4);
    E->image_scores = (float*)E->dmalloc((size_t)B * 4);
    E->rng_eb = (float*)E->dmalloc((size_t)B * 8 * 4);
    // cross-attention K/V buffers
    E->ctx_bf16 = (bf16_t*)E->dmalloc((size_t)E->halves * B * c.text_len * rup(c.unet_cross_dim, 8) * 2);
    for (auto& sl : E->cross_slots) {
      bf16_t* k = (bf16_t*)E->dmalloc((size_t)E->halves * B * c.text_len * sl.C * 2);
      bf16_t* v = (bf16_t*)E->dmalloc((size_t)E->halves * B * c.text_len * sl.C * 2);
      E->cross_kv.push_back({k, v});
    }
    if (!E->plan_only) HIPCHK(hipDeviceSynchronize());
    // the statistics fusions of every program, asked of the launcher's planner on the context its forward runs get
    {
      const auto& I = E->inst[0];
      char* const slab[dd_engine::NPROG] = {I.act[0], I.act[1], I.act[2], E->venc_slab, E->tower[0].slab, E->tower[1].slab};
      for (int p = 0; p < dd_engine::NPROG; ++p) {
        if (E->prog[p].ops.empty()) continue;      // not built
        Ctx pc = make_ctx(E, E->prog[p], slab[p], nullptr);
        if (p == dd_engine::UNET && c.unet_add_time_dim > 0) pc.img_bias = 2 * c.max_batch;
        resolve_fusions(E->prog[p], pc);
      }
    }
    E->finalized = true;
  } catch (const std::exception& ex) { E->err = ex.what(); return DD_ERR_HIP; }
  return DD_OK;
}

// the graph is built at finalize: until then the number of CFG halves is a setting
int dd_set_cfg_free(dd_engine* E, int on) {
  if (!E) return DD_ERR_ARG;
  if (E->finalized) { E->err = "dd_set_cfg_free after dd_finalize_weights: the UNet program is built for the batch it runs on"; return DD_ERR_STATE; }
  E->halves = on ? 1 : 2;
  return DD_OK;
}
int dd_cfg_free(dd_engine* E) { return E ? (E->halves == 1 ? 1 : 0) : DD_ERR_ARG; }

int dd_set_schedule(dd_engine* E, const int* timesteps, int n, const float* alphas_cumprod, int num_train, float final_alpha,
                    const dd_sampler_params* sp) {
  return dd_set_schedule_s(E, timesteps, n, alphas_cumprod, num_train, final_alpha, sp, 0);
}

int dd_set_schedule_s(dd_engine* E, const int* timesteps, int n, const float* alphas_cumprod, int num_train, float final_alpha,
                      const dd_sampler_params* sp, int solver) {
  return dd_set_schedule_e(E, timesteps, n, alphas_cumprod, num_train, final_alpha, sp, solver, 0.f);
}

int dd_set_schedule_e(dd_engine* E, const int* timesteps, int n, const float* alphas_cumprod, int num_train, float final_alpha,
                      const dd_sampler_params* sp, int solver, float eta) {
  return dd_set_schedule_sde(E, timesteps, n, alphas_cumprod, num_train, final_alpha, sp, solver, eta, 0.f);
}

int dd_set_schedule_sde(dd_engine* E, const int* timesteps, int n, const float* alphas_cumprod, int num_train, float final_alpha,
                        const dd_sampler_params* sp, int solver, float eta, float sde_eta) {
  if (!E || !timesteps || n < 1 || !alphas_cumprod || !sp) return DD_ERR_ARG;
  // sde_eta > 0 is SDE-DPM-Solver++(2M): solver 1 with eta = 0, one noise stream per step
  static_assert(DD_RNG_STEP_STREAMS == 4096, "the message below names the count");
  const char* bad = !(sde_eta >= 0.f && sde_eta <= 1.f) ? "sde_eta must be in [0, 1]"
                    : !(sde_eta > 0.f)                  ? nullptr
                    : eta > 0.f                         ? "sde_eta > 0 needs eta = 0: eta is the noise of stochastic DDIM (solver 0)"
                    : solver != 1                       ? "sde_eta > 0 is SDE-DPM-Solver++(2M): it needs solver 1"
                    : n > DD_RNG_STEP_STREAMS           ? "sde_eta > 0: at most 4096 steps (one noise stream per step)" : nullptr;
  if (bad) { E->err = bad; return DD_ERR_ARG; }
  if (!E->finalized) { E->err = "finalize first"; return DD_ERR_STATE; }
  DD_TRY(E, {
    const dd_config& c = E->cfg;
    if (sp->prediction_type < 0 || sp->prediction_type > 2) throw std::runtime_error("prediction_type must be 0 (epsilon), 1 (v_prediction) or 2 (sample)");
    if (!(sp->guidance_rescale >= 0.f && sp->guidance_rescale <= 1.f)) throw std::runtime_error("guidance_rescale must be in [0, 1]");
    if (E->halves == 1 && sp->guidance_rescale != 0.f)
      throw std::runtime_error("guidance_rescale != 0 on a CFG-free engine (dd_set_cfg_free): there is no guidance to rescale, the factor is identically 1 at m = c");
    if (solver < 0 || solver > 1) throw std::runtime_error("solver must be 0 (DDIM) or 1 (DPM-Solver++(2M))");
    if (!(eta >= 0.f && eta <= 1.f)) throw std::runtime_error("eta must be in [0, 1]");
    if (eta > 0.f && solver != 0) throw std::runtime_error("eta > 0 is stochastic DDIM (solver 0): the per-step noise of solver 1 is sde_eta (dd_set_schedule_sde)");
    if (eta > 0.f && n > DD_RNG_STEP_STREAMS) throw std::runtime_error("eta > 0: at most " + std::to_string(DD_RNG_STEP_STREAMS) + " steps (one noise stream per step)");
    // A complete new schedule is built beside the engine's own and swapped in at the end: a refusal, or an allocation that fails, leaves
    // the engine as it was.  `out` frees what it holds when this block is left -- the partial new one, or after the swap the old one
    struct Outgoing { dd_engine* E; Schedule S; ~Outgoing() { for (void* q : S.allocs) E->dfree(q); } } out{E, {}};
    Schedule& S = out.S;
    auto alloc = [&](size_t bytes, bool zero) { S.allocs.push_back(E->dmalloc(bytes, zero)); return (float*)S.allocs.back(); };
    auto upload = [&](const std::vector<float>& h) {
      float* d = alloc(h.size() * 4, false);
      HIPCHK(hipMemcpy(d, h.data(), h.size() * 4, hipMemcpyHostToDevice));
      return d;
    };
    S.solver = solver;
    S.rule = StepRule{sp->prediction_type, sde_eta > 0.f ? 2 : eta > 0.f ? 1 : 0, sde_eta > 0.f ? sde_eta : eta};
    const char* s_name = S.rule.noise == 2 ? "sde_eta" : "eta";
    std::vector<float> head((size_t)n * 4);      // coef[0..3] of every step, the same under both rules
    const int ratio = num_train / n;
    for (int i = 0; i < n; ++i) {
      const int t = timesteps[i], prev = t - ratio;
      if (t < 0 || t >= num_train) throw std::runtime_error("timestep out of range");
      const double a = alphas_cumprod[t], ap = prev >= 0 ? alphas_cumprod[prev] : final_alpha;
      const double a_before = i > 0 ? alphas_cumprod[timesteps[i - 1]] : 0.0;
      float* q = &head[(size_t)i * 4];
      q[0] = sp->guidance_scale; q[1] = (float)sqrt(a); q[2] = (float)sqrt(1 - a); q[3] = (float)sqrt(ap);
      StepRow row;
      if (sampler_step_row({sp->prediction_type, 0, 0.0}, i, n, a_before, a, ap, &row))      // the division form of the step divides by sqrt(a) as well
        throw std::runtime_error(sp->prediction_type == 0 ? "epsilon-prediction with alphas_cumprod = 0 at timestep " + std::to_string(t) +
                                 " (zero terminal SNR): x0 is undefined there" : "sample-prediction with alphas_cumprod = 1 at timestep " + std::to_string(t));
      S.det.row.push_back(row);
      if (!S.stochastic()) continue;
      if (sampler_step_row(S.rule, i, n, a_before, a, ap, &row))
        throw std::runtime_error(std::string(s_name) + " > 0: the step at timestep " + std::to_string(t) + " has no finite sigma");
      S.sto.row.push_back(row);
    }
    auto upload_rows = [&](Schedule::Rows& R) {
      std::vector<float> coef((size_t)n * 8, 0.f), lin((size_t)n * 4);
      for (int i = 0; i < n; ++i) {
        std::copy_n(&head[(size_t)i * 4], 4, &coef[(size_t)i * 8]);
        coef[(size_t)i * 8 + 4] = R.row[i].d;
        std::copy_n(R.row[i].lin, 4, &lin[(size_t)i * 4]);
      }
      R.coef = upload(coef); R.lin = upload(lin);
    };
    upload_rows(S.det);
    if (S.stochastic()) upload_rows(S.sto);
    if (S.keeps_history())
      S.x0_hist = alloc((size_t)c.max_batch * std::max({c.unet_in_channels, c.unet_out_channels, c.vae_latent_channels}) * c.latent_size * c.latent_size * 4, true);
    // sinusoidal timestep embedding (diffusers Timesteps: flip_sin_to_cos, freq_shift) on host, MLP + projections on GPU (fp32)
    const int C0 = c.unet_block_out_channels[0], half = C0 / 2, TE = C0 * 4;
    std::vector<float> sinus((size_t)n * C0);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < half; ++j) {
        const float freq = expf(-logf(10000.f) * (float)j / ((float)half - c.unet_freq_shift));
        const float a = (float)timesteps[i] * freq;
        const float sn = sinf(a), cs = cosf(a);
        if (c.unet_flip_sin_to_cos) { sinus[(size_t)i * C0 + j] = cs; sinus[(size_t)i * C0 + half + j] = sn; }
        else { sinus[(size_t)i * C0 + j] = sn; sinus[(size_t)i * C0 + half + j] = cs; }
      }
    float* d_sin = upload(sinus);
    float* d_h1 = alloc((size_t)n * TE * 4, false);
    S.d_emb = alloc((size_t)n * TE * 4, false);
    HIPCHK(launch_linear_f32(d_sin, E->temb_w1, E->temb_b1, d_h1, n, TE, C0, 0, nullptr));
    HIPCHK(launch_linear_f32(d_h1, E->temb_w2, E->temb_b2, S.d_emb, n, TE, TE, 1, nullptr));
    for (ConvW* cw : E->temb_convs) {
      float* table = alloc((size_t)n * cw->Cout * 4, false);
      HIPCHK(launch_linear_f32(S.d_emb, cw->temb_w, cw->temb_b, table, n, cw->Cout, TE, 1, nullptr));
      if (cw->bias) HIPCHK(launch_add_rowvec_f32(table, cw->bias, n, cw->Cout, nullptr));   // + conv1.bias
      S.temb_bias.push_back({table, c.unet_add_time_dim > 0 ? alloc((size_t)n * 2 * c.max_batch * cw->Cout * 4, false) : nullptr});
    }
    // the new tables are complete and nothing in flight reads the old ones: from here on the engine's schedule is replaced
    HIPCHK(hipDeviceSynchronize());
    std::swap(E->sched, S);
    E->timesteps.assign(timesteps, timesteps + n);
    E->sp = *sp;
    E->added_cond_set = false;
    for (size_t k = 0; k < E->temb_convs.size(); ++k) {
      E->temb_convs[k]->bias_table = E->sched.temb_bias[k].first;
      E->temb_convs[k]->bias_table_img = E->sched.temb_bias[k].second;
    }
  });
}

int dd_set_prototypes(dd_engine* E, const float* Pc, const float* Pg, int C, int K, int D) {
  if (!E || C < 1 || D < 1) return DD_ERR_ARG;
  DD_TRY(E, {
    E->pC = C; E->pK = K; E->pD = D;
    HIPCHK(hipDeviceSynchronize());
    E->dfree(E->Pc); E->dfree(E->Pg);
    E->Pc = nullptr; E->Pg = nullptr;
    if (Pc) { E->Pc = (float*)E->dmalloc((size_t)C * D * 4, false); HIPCHK(hipMemcpy(E->Pc, Pc, (size_t)C * D * 4, hipMemcpyHostToDevice)); }
    if (Pg) { E->Pg = (float*)E->dmalloc((size_t)C * K * D * 4, false); HIPCHK(hipMemcpy(E->Pg, Pg, (size_t)C * K * D * 4, hipMemcpyHostToDevice)); }
  });
}

int dd_set_prompt(dd_engine* E, const float* embeds, int B, void* stream) {
  if (!E || !embeds) return DD_ERR_ARG;
  DD_TRY(E, {
    check_batch(E, B);
    const dd_config& c = E->cfg;
    hipStream_t s = (hipStream_t)stream;
    const int rows = E->halves * B * c.text_len, ld = rup(c.unet_cross_dim, 8);      // a CFG-free engine: [B, T, D], conditional only
    // [rows, cross_dim] fp32 -> bf16 rows (treated as NCHW with H*W = 1 per row)
    HIPCHK(launch_nchw_f32_to_nhwc_bf16(embeds, E->ctx_bf16, rows, c.unet_cross_dim, 1, 1, ld, ld, 0, 1.f, s));
    for (size_t i = 0; i < E->cross_slots.size(); ++i) {
      auto& sl = E->cross_slots[i];
      ConvW* const proj[2] = {sl.wk, sl.wv};
      bf16_t* const kv[2] = {E->cross_kv[i].first, E->cross_kv[i].second};
      for (int j = 0; j < 2; ++j) {
        ConvW* w = proj[j];
        ConvGemmParams p; memset(&p, 0, sizeof p);
        p.alpha = 1.f; p.partial = (float*)E->scratch_partial;
        p.x = E->ctx_bf16; p.x_ld = ld; p.w = w->w_fwd; p.taptab = w->tap_fwd;
        p.y = kv[j]; p.y_ld = sl.C;
        p.B = 1; p.H = rows; p.W = 1; p.Ho = rows; p.Wo = 1; p.stride = 1;
        p.cin = w->sf.cin; p.ntaps = w->sf.ntaps; p.M = rows; p.N = w->sf.N; p.K = w->sf.K;
        HIPCHK(launch_conv_gemm(p, E->partial_cap, s));
      }
    }
  });
}

int dd_set_added_cond(dd_engine* E, const float* text_embeds, const float* time_ids, int B, void* stream) {
  if (!E || !text_embeds || !time_ids) return DD_ERR_ARG;
  DD_TRY(E, {
    check_batch(E, B);
    const dd_config& c = E->cfg;
    if (c.unet_add_time_dim <= 0) throw std::runtime_error("this UNet has no additional conditioning (unet_add_time_dim == 0)");
    if (!E->sched.d_emb) throw std::runtime_error("dd_set_schedule first");
    hipStream_t s = (hipStream_t)stream;
    const int nb = 2 * B, n = (int)E->timesteps.size(), TE = c.unet_block_out_channels[0] * 4;
    const int Dt = c.unet_add_text_dim, Ds = 6 * c.unet_add_time_dim, Din = Dt + Ds;
    // scratch (setup path: plain allocations, freed at the end)
    float* cat = nullptr; float* h1 = nullptr; float* aug = nullptr; float* X = nullptr;
    HIPCHK(hipMalloc((void**)&cat, (size_t)nb * Din * 4)); HIPCHK(hipMalloc((void**)&h1, (size_t)nb * TE * 4));
    HIPCHK(hipMalloc((void**)&aug, (size_t)nb * TE * 4)); HIPCHK(hipMalloc((void**)&X, (size_t)n * nb * TE * 4));
    // cat[text_embeds, add_time_proj(time_ids).reshape(B, -1)]
    HIPCHK(hipMemcpy2DAsync(cat, (size_t)Din * 4, text_embeds, (size_t)Dt * 4, (size_t)Dt * 4, nb, hipMemcpyDeviceToDevice, s));
    for (int k = 0; k < 6; ++k) {
      // time id k of every image -> columns [Dt + k*dim, Dt + (k+1)*dim): gather the k-th id with a strided copy first
      HIPCHK(hipMemcpy2DAsync(h1, 4, time_ids + k, 6 * 4, 4, nb, hipMemcpyDeviceToDevice, s));
      HIPCHK(launch_sinusoid_f32(h1, cat, nb, c.unet_add_time_dim, Din, Dt + k * c.unet_add_time_dim, 1, s));
    }
    HIPCHK(launch_linear_f32(cat, E->add_w1, E->add_b1, h1, nb, TE, Din, 0, s));
    HIPCHK(launch_linear_f32(h1, E->add_w2, E->add_b2, aug, nb, TE, TE, 1, s));
    HIPCHK(launch_add_outer_f32(E->sched.d_emb, aug, X, n, nb, TE, s));                 // emb[step, image] = time_embedding(t) + aug_emb
    for (ConvW* cw : E->temb_convs) {
      HIPCHK(launch_linear_f32(X, cw->temb_w, cw->temb_b, cw->bias_table_img, n * nb, cw->Cout, TE, 1, s));
      if (cw->bias) HIPCHK(launch_add_rowvec_f32(cw->bias_table_img, cw->bias, n * nb, cw->Cout, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    hipFree(cat); hipFree(h1); hipFree(aug); hipFree(X);
    E->added_cond_set = true;
  });
}

int dd_add_noise(dd_engine* E, const float* x, const float* noise, float* out, int B, int step_index, void* stream) {
  if (!E || !x || !noise || !out) return DD_ERR_ARG;
  DD_TRY(E, {
    if (step_index < 0 || step_index >= (int)E->timesteps.size()) throw std::runtime_error("step_index out of range");
    const dd_config& c = E->cfg;
    // coef[step][1..2] = sqrt(a_t), sqrt(1-a_t)
    HIPCHK(launch_axpby(x, noise, out, (size_t)B * c.unet_in_channels * c.latent_size * c.latent_size,
                        E->sched.det.coef + (size_t)step_index * 8 + 1, (hipStream_t)stream));
  });
}

int dd_unet_forward(dd_engine* E, const float* z, int step_index, float* eps2_out, int B, void* stream) {
  if (!E || !z || !eps2_out) return DD_ERR_ARG;
  DD_TRY(E, {
    check_batch(E, B);
    const dd_config& c = E->cfg;
    hipStream_t s = (hipStream_t)stream;
    unet_fwd(E, 0, z, step_index, s);
    const Tn& out = E->unet.t[E->unet_out];
    HIPCHK(launch_nhwc_to_nchw_f32(E->inst[0].act[dd_engine::UNET] + out.off, 1, eps2_out, E->halves * B, c.unet_out_channels, c.latent_size, c.latent_size, out.ld,
                                   1.f, 0.f, 0, 0.f, 0.f, s));
  });
}

// the launch sequence of one plain step: UNet forward (no stash) + CFG + scheduler step (x0_prev: the history of a DPM-Solver++(2M) step)
static void denoise_step_enqueue(dd_engine* E, const float* z, int step_index, const float* x0_prev, float* z_prev_out, float* x0_out,
                                 hipStream_t s, const StepNoise& sn) {
  unet_fwd(E, 0, z, step_index, s, /*stash=*/false);
  sampler_step(E, 0, z, step_index, x0_prev, z_prev_out, x0_out, s, sn);
}

int dd_denoise_step(dd_engine* E, const float* z, int step_index, float* z_prev_out, float* x0_out, int B, void* stream) {
  return dd_denoise_step_h(E, z, step_index, nullptr, z_prev_out, x0_out, B, stream);
}

// one plain step with its optional inputs: the history (solver 1), the noise (eta > 0) or both (sde_eta > 0); the public calls and dd_expand's loop are this
static int denoise_step_call(dd_engine* E, const float* z, int step_index, const float* x0_prev, const StepNoise& sn, float* z_prev_out,
                             float* x0_out, int B, void* stream) {
  if (!E || !z || !z_prev_out) return DD_ERR_ARG;
  if (history_refused(E, x0_prev) || noise_refused(E, sn.noise)) return DD_ERR_STATE;
  DD_TRY(E, {
    check_batch(E, B);
    if (step_index < 0 || step_index >= (int)E->timesteps.size()) throw std::runtime_error("step_index out of range");
    denoise_step_enqueue(E, z, step_index, x0_prev, z_prev_out, x0_out, (hipStream_t)stream, sn);
  });
}

int dd_denoise_step_h(dd_engine* E, const float* z, int step_index, const float* x0_prev, float* z_prev_out, float* x0_out, int B,
                      void* stream) {
  return denoise_step_call(E, z, step_index, x0_prev, StepNoise(), z_prev_out, x0_out, B, stream);
}

int dd_denoise_step_n(dd_engine* E, const float* z, int step_index, const float* step_noise, float* z_prev_out, float* x0_out, int B,
                      void* stream) {
  StepNoise sn;
  sn.noise = step_noise;
  return denoise_step_call(E, z, step_index, nullptr, sn, z_prev_out, x0_out, B, stream);
}

int dd_denoise_step_hn(dd_engine* E, const float* z, int step_index, const float* x0_prev, const float* step_noise, float* z_prev_out,
                       float* x0_out, int B, void* stream) {
  StepNoise sn;
  sn.noise = step_noise;
  return denoise_step_call(E, z, step_index, x0_prev, sn, z_prev_out, x0_out, B, stream);
}

int dd_decode(dd_engine* E, const float* z, float* image_out, int denormalize, int B, void* stream) {
  if (!E || !z || !image_out) return DD_ERR_ARG;
  DD_TRY(E, {
    check_batch(E, B);
    const dd_config& c = E->cfg;
    hipStream_t s = (hipStream_t)stream;
    vae_fwd(E, 0, z, s);
    const Tn& img = E->vae.t[E->vae_out];
    HIPCHK(launch_nhwc_to_nchw_f32(E->inst[0].act[dd_engine::VAE] + img.off, 1, image_out, B, c.vae_out_channels, img.H, img.W, img.ld,
                                   denormalize ? 0.5f : 1.f, denormalize ? 0.5f : 0.f, denormalize, 0.f, 1.f, s));
  });
}

int dd_vae_encode(dd_engine* E, const float* images, const float* noise, float* latents_out, float* moments_out, int B, void* stream) {
  if (!E || !images || !latents_out) return DD_ERR_ARG;
  DD_TRY(E, {
    check_batch(E, B);
    if (!E->venc_slab) throw std::runtime_error("no VAE encoder weights were loaded (vae/encoder.* keys)");
    const dd_config& c = E->cfg;
    hipStream_t s = (hipStream_t)stream;
    Ctx ctx = make_ctx(E, E->venc, E->venc_slab, s);
    ctx.stash = false;
    const Tn& in = E->venc.t[E->venc_in];
    HIPCHK(launch_nchw_f32_to_nhwc_bf16(images, act_ptr(ctx, in), B, c.vae_out_channels, in.H, in.W, in.ld, in.ld, 0, 1.f, s));
    run_fwd(E->venc, ctx);
    const Tn& mo = E->venc.t[E->venc_out];
    HIPCHK(launch_vae_sample((const float*)(ctx.act + mo.off), mo.ld, noise, latents_out, moments_out, B, c.vae_latent_channels,
                             mo.H * mo.W, c.vae_scaling_factor, s));
  });
}

int dd_text_encode_tower(dd_engine* E, int which, const int* input_ids, float* hidden_out, float* pooled_out, int n, void* stream) {
  if (!E || !input_ids || (!hidden_out && !pooled_out) || which < 0 || which > 1) return DD_ERR_ARG;
  DD_TRY(E, {
    if (!E->finalized) throw std::runtime_error("dd_finalize_weights has not been called");
    const dd_engine::TextTower& tw = E->tower[which];
    const char* const missing[2] = {"no text encoder weights were loaded (text/text_model.* keys)", "no second text tower was loaded (text2/text_model.* keys)"};
    if (!tw.slab) throw std::runtime_error(missing[which]);
    if (n < 1 || n > E->text_batch) throw std::runtime_error("dd_text_encode: n must be in [1, 2*max_batch]");
    if (pooled_out && (which != 1 || !tw.proj_w)) throw std::runtime_error("pooled text embeddings come from the second tower's text_projection (text2/text_projection.weight)");
    const dd_config& c = E->cfg;
    hipStream_t s = (hipStream_t)stream;
    const Program& P = E->prog[dd_engine::TEXT + which];
    const int T = c.text_len, Cc = tw.hidden;
    HIPCHK(hipMemsetAsync(E->text_ids, 0, (size_t)E->text_batch * T * 4, s));
    HIPCHK(hipMemcpyAsync(E->text_ids, input_ids, (size_t)n * T * 4, hipMemcpyDeviceToDevice, s));
    Ctx ctx = make_ctx(E, P, tw.slab, s);
    ctx.stash = false;
    const Tn& in = P.t[tw.in];
    HIPCHK(launch_clip_embed(E->text_ids, tw.tok_emb, tw.pos_emb, act_ptr(ctx, in), in.ld, in.rows, T, Cc, tw.vocab, s));
    run_fwd(P, ctx);
    if (hidden_out) {
      const Tn& o = P.t[tw.out];
      HIPCHK(launch_rows_bf16_to_f32(act_ptr(ctx, o), o.ld, hidden_out, n * T, Cc, s));
    }
    if (pooled_out) {
      const Tn& f = P.t[tw.fin];
      HIPCHK(launch_clip_pool_project(E->text_ids, act_ptr(ctx, f), f.ld, tw.proj_w, pooled_out, n, T, Cc, tw.proj, s));
    }
  });
}

int dd_text_encode(dd_engine* E, const int* input_ids, float* embeds_out, int n, void* stream) {
  if (!E || !input_ids || !embeds_out) return DD_ERR_ARG;
  if (E->tower[1].slab) { E->err = "this model has two text towers: use dd_text_encode_tower"; return DD_ERR_STATE; }
  return dd_text_encode_tower(E, 0, input_ids, embeds_out, nullptr, n, stream);
}

int dd_guide_encode_pooled(dd_engine* E, const float* images, float* feats, int B, int use_max, void* stream) {
  if (!E || !images || !feats) return DD_ERR_ARG;
  DD_TRY(E, {
    check_batch(E, B);
    if (use_max && E->cfg.guide_kind == 1) throw std::runtime_error("the ViT guide has no spatial pooling (encode_image = the projected class token)");
    const dd_config& c = E->cfg;
    hipStream_t s = (hipStream_t)stream;
    Ctx gc = make_ctx(E, dd_engine::GUIDE, 0, s);
    const Tn& gin = E->guide.t[E->guide_in];
    HIPCHK(launch_nchw_to_nhwc_f32(images, act_f32(gc, gin), B, 3, gin.H, gin.W, gin.ld, gin.ld, s));
    run_fwd(E->guide, gc);
    guide_features_out(E, gc, feats, s, use_max);
  });
}

int dd_guide_encode(dd_engine* E, const float* images, float* feats, int B, void* stream) {
  return dd_guide_encode_pooled(E, images, feats, B, 0, stream);
}

int dd_transform_guidance(dd_engine* E, const float* z, const int* targets, const float* ch_e, const float* ch_b, int first_step_index,
                          int P, float* z_out, float* score_out, float* grad_eb_out, int B, void* stream) {
  if (!E || !z || !targets || !ch_e || !ch_b || !z_out || P < 1) return DD_ERR_ARG;
  DD_TRY(E, {
    check_batch(E, B, /*need_grad=*/true);
    const dd_config& c = E->cfg;
    if (P > (int)E->inst.size()) throw std::runtime_error("guidance period exceeds max_guidance_period");
    if (first_step_index < 0 || first_step_index + P > (int)E->timesteps.size()) throw std::runtime_error("guide steps out of range");
    if ((E->sp.use_global && !E->Pc) || (E->sp.use_local && !E->Pg)) throw std::runtime_error("prototypes not set");
    hipStream_t s = (hipStream_t)stream;
    const int BC = B * c.unet_in_channels, HW = c.latent_size * c.latent_size;
    float* score = score_out ? score_out : E->score_tmp;
    HIPCHK(hipMemsetAsync(score, 0, sizeof(float), s));
    HIPCHK(hipMemsetAsync(E->image_scores, 0, (size_t)B * sizeof(float), s));
    // z0 = z*(1+e)+b  (generate_data.py:696)
    HIPCHK(launch_affine(z, ch_e, ch_b, E->inst[0].z_in, BC, HW, s));
    const float weight = 1.f / (float)E->sp.guidance_period;   // score / args.guidance_period (:719)
    for (int k = 0; k < P; ++k) {
      const float* zin = E->inst[k].z_in;
      // the chained look-ahead steps are first-order and deterministic under every schedule: their reverse pass differentiates them
      guided_forward(E, k, zin, first_step_index + k, targets, 0, weight, score, s, /*x0_prev=*/nullptr, DETERMINISTIC);
      if (k + 1 < P) HIPCHK(hipMemcpyAsync(E->inst[k + 1].z_in, E->inst[k].z_next, (size_t)BC * HW * 4, hipMemcpyDeviceToDevice, s));
    }
    float* g_next = nullptr;
    float* gbuf[2] = {E->f32_tmp[0], E->f32_tmp[1]};
    for (int k = P - 1; k >= 0; --k) {
      float* g_z = gbuf[k & 1];
      guided_backward(E, k, first_step_index + k, g_next, g_z, E->f32_tmp[2], s);
      g_next = g_z;
    }
    if (grad_eb_out) HIPCHK(hipMemcpyAsync(grad_eb_out, g_next, (size_t)BC * HW * 4, hipMemcpyDeviceToDevice, s));
    // e -= rho*ge ; b -= rho*gb ; z' = clamp(z*(1+e)+b, z-c, z+c)  (:721-728)
    HIPCHK(launch_transform_update(z, g_next, ch_e, ch_b, z_out, BC, HW, E->sp.rho, E->sp.constraint_value, s));
  });
}

int dd_direct_guidance(dd_engine* E, const float* z, const int* targets, int step_index, float* z_next_out, float* x0_out,
                       float* score_out, float* grad_z_out, int B, void* stream) {
  return dd_direct_guidance_h(E, z, targets, step_index, nullptr, z_next_out, x0_out, score_out, grad_z_out, B, stream);
}

static int direct_guidance_call(dd_engine* E, const float* z, const int* targets, int step_index, const float* x0_prev, const StepNoise& sn,
                                float* z_next_out, float* x0_out, float* score_out, float* grad_z_out, int B, void* stream);
int dd_direct_guidance_h(dd_engine* E, const float* z, const int* targets, int step_index, const float* x0_prev, float* z_next_out,
                         float* x0_out, float* score_out, float* grad_z_out, int B, void* stream) {
  return direct_guidance_call(E, z, targets, step_index, x0_prev, StepNoise(), z_next_out, x0_out, score_out, grad_z_out, B, stream);
}

int dd_direct_guidance_n(dd_engine* E, const float* z, const int* targets, int step_index, const float* step_noise, float* z_next_out,
                         float* x0_out, float* score_out, float* grad_z_out, int B, void* stream) {
  StepNoise sn;
  sn.noise = step_noise;
  return direct_guidance_call(E, z, targets, step_index, nullptr, sn, z_next_out, x0_out, score_out, grad_z_out, B, stream);
}

int dd_direct_guidance_hn(dd_engine* E, const float* z, const int* targets, int step_index, const float* x0_prev, const float* step_noise,
                          float* z_next_out, float* x0_out, float* score_out, float* grad_z_out, int B, void* stream) {
  StepNoise sn;
  sn.noise = step_noise;
  return direct_guidance_call(E, z, targets, step_index, x0_prev, sn, z_next_out, x0_out, score_out, grad_z_out, B, stream);
}

// direct guidance with its optional inputs, as denoise_step_call
static int direct_guidance_call(dd_engine* E, const float* z, const int* targets, int step_index, const float* x0_prev, const StepNoise& sn,
                                float* z_next_out, float* x0_out, float* score_out, float* grad_z_out, int B, void* stream) {
  if (!E || !z || !targets || !z_next_out) return DD_ERR_ARG;
  if (history_refused(E, x0_prev) || noise_refused(E, sn.noise)) return DD_ERR_STATE;
  DD_TRY(E, {
    check_batch(E, B, /*need_grad=*/true);
    const dd_config& c = E->cfg;
    if (step_index < 0 || step_index >= (int)E->timesteps.size()) throw std::runtime_error("step_index out of range");
    if ((E->sp.use_global && !E->Pc) || (E->sp.use_local && !E->Pg)) throw std::runtime_error("prototypes not set");
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)B * c.unet_in_channels * c.latent_size * c.latent_size;
    float* score = score_out ? score_out : E->score_tmp;
    HIPCHK(hipMemsetAsync(score, 0, sizeof(float), s));
    HIPCHK(hipMemsetAsync(E->image_scores, 0, (size_t)B * sizeof(float), s));
    HIPCHK(hipMemcpyAsync(E->inst[0].z_in, z, n * 4, hipMemcpyDeviceToDevice, s));
    guided_forward(E, 0, E->inst[0].z_in, step_index, targets, 1, 1.f, score, s, x0_prev, sn);
    float* g_z = E->f32_tmp[0];
    guided_backward(E, 0, step_index, nullptr, g_z, E->f32_tmp[2], s);
    if (grad_z_out) HIPCHK(hipMemcpyAsync(grad_z_out, g_z, n * 4, hipMemcpyDeviceToDevice, s));
    if (x0_out) HIPCHK(hipMemcpyAsync(x0_out, E->inst[0].x0, n * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(launch_sub_scaled(E->inst[0].z_next, g_z, z_next_out, n, E->sp.rho, s));   // :762
  });
}

// out [B, n_per_unit] of one stream of the counter-based generator; the unit ids travel in the kernel arguments, DD_RNG_UNITS per launch
static void philox_units_enqueue(uint64_t seed, int rng_stream, const uint64_t* unit_ids, int B, int64_t n_per_unit, float* out, hipStream_t s) {
  HIPCHK(for_rng_unit_ranges(unit_ids, B, [&](const RngUnits& ids, int u0, int cnt) {
    return launch_philox_units(ids, cnt, seed, rng_stream, n_per_unit, out + (size_t)u0 * n_per_unit, s);
  }));
}

int dd_randn_units(dd_engine* E, uint64_t seed, int rng_stream, const uint64_t* unit_ids, int B, int64_t n_per_unit, float* out, void* stream) {
  if (!E || !unit_ids || !out || B < 1 || n_per_unit < 1 || !rng_stream_ok(rng_stream)) return DD_ERR_ARG;
  DD_TRY(E, { philox_units_enqueue(seed, rng_stream, unit_ids, B, n_per_unit, out, (hipStream_t)stream); });
}

// noise_mode 1 of dd_expand: the loop's first latent written straight from the generated values into `z0`, e and b into E->rng_eb
static int expand_generated_inputs(dd_engine* E, const dd_expand_args* a, float* z0, hipStream_t s) {
  DD_TRY(E, {
    check_batch(E, a->B);
    const dd_config& c = E->cfg;
    const int HW = c.latent_size * c.latent_size;
    if (a->text_to_img) {
      philox_units_enqueue(a->seed, 0, a->unit_ids, a->B, (int64_t)c.unet_in_channels * HW, z0, s);      // z = n * init_noise_sigma (= 1 for DDIM)
    } else {
      HIPCHK(for_rng_unit_ranges(a->unit_ids, a->B, [&](const RngUnits& ids, int u0, int cnt) {
        const size_t off = (size_t)u0 * c.unet_in_channels * HW;
        return launch_philox_add_noise(ids, cnt, a->seed, a->image_latents + off, z0 + off, c.unet_in_channels, HW, a->offset_noise,
                                       E->sched.det.coef + (size_t)a->start_index * 8 + 1, s);
      }));
    }
    if (a->guidance_type == 1) {
      philox_units_enqueue(a->seed, 2, a->unit_ids, a->B, 4, E->rng_eb, s);
      philox_units_enqueue(a->seed, 3, a->unit_ids, a->B, 4, E->rng_eb + (size_t)a->B * 4, s);
    }
  });
}

int dd_expand(dd_engine* E, const dd_expand_args* a, void* stream) {
  if (!E || !a || !a->z_out || a->noise_mode < 0 || a->noise_mode > 1) return DD_ERR_ARG;
  if ((!a->image_latents && !a->text_to_img) || (a->noise_mode == 0 && !a->noise) || (a->noise_mode == 1 && !a->unit_ids)) return DD_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int n = (int)E->timesteps.size();
  if (a->start_index < 0 || a->start_index >= n) { E->err = "start_index out of range"; return DD_ERR_ARG; }
  if (a->text_to_img && a->start_index != 0) { E->err = "text_to_img runs the whole schedule: start_index must be 0"; return DD_ERR_ARG; }
  // eta > 0 or sde_eta > 0: the noise of step i of row k is generated from (seed, unit_ids[k], stream 16 + i) in either noise_mode
  StepNoise sn;
  if (E->sched.stochastic()) {
    if (!a->unit_ids) { E->err = std::string("this schedule was set with ") + (E->sched.rule.noise == 1 ? "eta" : "sde_eta") + " > 0: dd_expand needs unit_ids (with seed they key the noise of every step)"; return DD_ERR_ARG; }
    sn.unit_ids = a->unit_ids; sn.seed = a->seed;
  }
  const float* ch_e = a->e;
  const float* ch_b = a->b;
  int rc;
  if (a->noise_mode == 1) {
    rc = expand_generated_inputs(E, a, E->f32_tmp[3], s);
    ch_e = E->rng_eb;
    ch_b = E->rng_eb + (size_t)a->B * 4;
  } else if (a->text_to_img) {
    // the caller's noise is the first latent (init_noise_sigma = 1): add_noise is skipped
    DD_TRY_RC(E, rc, {
      check_batch(E, a->B);
      const dd_config& c = E->cfg;
      HIPCHK(hipMemcpyAsync(E->f32_tmp[3], a->noise, (size_t)a->B * c.unet_in_channels * c.latent_size * c.latent_size * 4, hipMemcpyDeviceToDevice, s));
    });
  } else {
    rc = dd_add_noise(E, a->image_latents, a->noise, E->f32_tmp[3], a->B, a->start_index, stream);
  }
  if (rc) return rc;
  float* cur = E->f32_tmp[3];
  float* nxt = E->f32_tmp[4];
  // DPM-Solver++(2M): every step leaves its x0 in the one history buffer (read and written in place); `hist` is that buffer once it
  // holds x0 of step i - 1 on the trajectory `cur` is on.  Under DDIM both stay null and the calls are those of version 8.
  float* const keep = E->sched.keeps_history() ? E->sched.x0_hist : nullptr;
  const float* hist = nullptr;
  for (int i = a->start_index; i < n; ++i) {
    const float* h = i == n - 1 ? nullptr : hist;          // the final step is first-order
    if (a->guidance_type == 1 && a->guide_count > 0 && i == a->guide_first) {
      // transform guidance at t == guide_timesteps[0], then the step is executed again from the corrected latent (:1203-1207): the
      // correction moved the latent off the trajectory the history belongs to, so that step runs without one
      rc = dd_transform_guidance(E, cur, a->targets, ch_e, ch_b, a->guide_first, a->guide_count, nxt, a->score_out, nullptr, a->B, stream);
      if (rc) return rc;
      std::swap(cur, nxt);
      rc = denoise_step_call(E, cur, i, nullptr, sn, nxt, keep, a->B, stream);
    } else if (a->guidance_type == 2 && i >= a->guide_first && i < a->guide_first + a->guide_count) {
      rc = direct_guidance_call(E, cur, a->targets, i, h, sn, nxt, keep, a->score_out, nullptr, a->B, stream);
    } else {
      rc = denoise_step_call(E, cur, i, h, sn, nxt, keep, a->B, stream);
    }
    if (rc) return rc;
    hist = keep;
    std::swap(cur, nxt);
  }
  DD_TRY_RC(E, rc, {
    const dd_config& c = E->cfg;
    HIPCHK(hipMemcpyAsync(a->z_out, cur, (size_t)a->B * c.unet_in_channels * c.latent_size * c.latent_size * 4, hipMemcpyDeviceToDevice, s));
  });
  if (rc) return rc;
  if (a->image_out) return dd_decode(E, cur, a->image_out, 1, a->B, stream);
  return DD_OK;
}

int dd_set_sample_weights(dd_engine* E, const float* w_host, int B) {
  if (!E) return DD_ERR_ARG;
  DD_TRY(E, {
    check_batch(E, B);
    E->sample_w_set = w_host != nullptr;
    if (w_host) {
      HIPCHK(hipDeviceSynchronize());   // a previous guidance call may still be reading the weights
      HIPCHK(hipMemcpy(E->sample_w, w_host, (size_t)B * sizeof(float), hipMemcpyHostToDevice));
    }
  });
}

int dd_get_image_scores(dd_engine* E, float* scores_out, int B, void* stream) {
  if (!E || !scores_out) return DD_ERR_ARG;
  DD_TRY(E, {
    check_batch(E, B);
    HIPCHK(hipMemcpyAsync(scores_out, E->image_scores, (size_t)B * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  });
}

// ---- per-module VJP diagnostics (parity tests of the hand-derived reverse programs against torch.autograd) ----
int dd_unet_vjp(dd_engine* E, const float* z, int step_index, const float* g_eps2, float* g_z_out, int B, void* stream) {
  if (!E || !z || !g_eps2 || !g_z_out) return DD_ERR_ARG;
  DD_TRY(E, {
    check_batch(E, B, /*need_grad=*/true);
    const dd_config& c = E->cfg;
    hipStream_t s = (hipStream_t)stream;
    const int HW = c.latent_size * c.latent_size;
    unet_fwd(E, 0, z, step_index, s);
    Ctx uc = make_ctx(E, dd_engine::UNET, 0, s);
    uc.step_index = step_index;
    const Tn& out = E->unet.t[E->unet_out];
    const float* cs = cot_normalise(E, g_eps2, (size_t)E->halves * B * c.unet_out_channels, HW, HW, s);
    HIPCHK(launch_nchw_f32_to_nhwc_bf16(g_eps2, grad_ptr(uc, out), E->halves * B, c.unet_out_channels, c.latent_size, c.latent_size, out.ld, out.ld, 0,
                                        1.f, s, cs));
    run_bwd(E->unet, uc);
    const Tn& in = E->unet.t[E->unet_in];
    HIPCHK(launch_dup_bwd(grad_ptr(uc, in), in.ld, g_z_out, B, c.unet_in_channels, HW, 0, in.B == 2 * B ? 2 : 1, s, cot_inv(cs)));
  });
}

int dd_decode_vjp(dd_engine* E, const float* z, const float* g_image, float* g_z_out, int B, void* stream) {
  if (!E || !z || !g_image || !g_z_out) return DD_ERR_ARG;
  DD_TRY(E, {
    check_batch(E, B, /*need_grad=*/true);
    const dd_config& c = E->cfg;
    hipStream_t s = (hipStream_t)stream;
    vae_fwd(E, 0, z, s);
    Ctx vc = make_ctx(E, dd_engine::VAE, 0, s);
    const Tn& img = E->vae.t[E->vae_out];
    const float* cs = cot_normalise(E, g_image, (size_t)B * c.vae_out_channels, img.H * img.W, img.H * img.W, s);
    HIPCHK(launch_nchw_f32_to_nhwc_bf16(g_image, grad_ptr(vc, img), B, c.vae_out_channels, img.H, img.W, img.ld, img.ld, 0, 1.f, s, cs));
    run_bwd(E->vae, vc);
    const Tn& vin = E->vae.t[E->vae_in];
    HIPCHK(launch_nhwc_to_nchw_f32(grad_ptr(vc, vin), 0, g_z_out, B, c.vae_latent_channels, c.latent_size, c.latent_size, vin.ld,
                                   1.f / c.vae_scaling_factor, 0.f, 0, 0.f, 0.f, s, cot_inv(cs)));
  });
}

int dd_guide_vjp(dd_engine* E, const float* images, const float* g_feats, float* g_images_out, int B, void* stream) {
  if (!E || !images || !g_feats || !g_images_out) return DD_ERR_ARG;
  DD_TRY(E, {
    check_batch(E, B, /*need_grad=*/true);
    const dd_config& c = E->cfg;
    hipStream_t s = (hipStream_t)stream;
    Ctx gc = make_ctx(E, dd_engine::GUIDE, 0, s);
    const Tn& gin = E->guide.t[E->guide_in];
    HIPCHK(launch_nchw_to_nhwc_f32(images, act_f32(gc, gin), B, 3, gin.H, gin.W, gin.ld, gin.ld, s));
    run_fwd(E->guide, gc);
    const float* cs = guide_features_grad_in(E, gc, g_feats, s);
    run_bwd(E->guide, gc);
    HIPCHK(launch_nhwc_to_nchw_f32(grad_f32(gc, gin), 1, g_images_out, B, 3, gin.H, gin.W, gin.ld, 1.f, 0.f, 0, 0.f, 0.f, s, cot_inv(cs)));
  });
}

int dd_profile_enable(dd_engine* E, int on) {
  if (!E) return DD_ERR_ARG;
  E->prof.on = on != 0;
  E->prof.used = 0;
  E->prof.chain = false;
  E->prof.recs.clear();
  return DD_OK;
}
// out[fam*3 + {0,1,2}] = {total ms, algorithmic flops, launches(op count)} for fam in {conv_gemm, attention, norm, other}
int dd_profile_read(dd_engine* E, double* out12) {
  if (!E || !out12) return DD_ERR_ARG;
  DD_TRY(E, {
    HIPCHK(hipDeviceSynchronize());
    for (int i = 0; i < 12; ++i) out12[i] = 0;
    FILE* dump = getenv("DD_PROFILE_DUMP") ? fopen(getenv("DD_PROFILE_DUMP"), "w") : nullptr;
    if (dump) fprintf(dump, "fam,bwd,M,N,K,flops,ms\n");
    for (auto& r : E->prof.recs) {
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, E->prof.pool[r.e0], E->prof.pool[r.e1]));
      if (dump) fprintf(dump, "%d,%d,%d,%d,%d,%.0f,%.5f\n", r.fam, r.bwd, r.M, r.N, r.K, r.flops, ms);
      out12[r.fam * 3 + 0] += ms; out12[r.fam * 3 + 1] += r.flops; out12[r.fam * 3 + 2] += 1;
    }
    if (dump) fclose(dump);
    E->prof.used = 0; E->prof.chain = false; E->prof.recs.clear();
  });
}

// ---- debug introspection: copy activation / gradient of tensor `idx` of program `prog` (0 unet, 1 vae, 2 guide; + 16 * instance)
// to a HOST fp32 buffer [rows*ld]; info4 = {rows, C, ld, is_f32}. Synchronises.
int dd_debug_tensor(dd_engine* E, int prog_inst, int idx, int want_grad, float* host_out, int* info4) {
  const int prog = prog_inst & 15, k = prog_inst >> 4;   // bits 4.. select the instance (chained guided step) of an activation
  if (!E || prog < 0 || prog > 2 || k < 0 || k >= (int)E->inst.size()) return DD_ERR_ARG;
  DD_TRY(E, {
    const Program& P = E->prog[prog];
    if (idx < 0) idx += (int)P.t.size();   // negative: from the end (-1 = the program's output tensor)
    if (idx < 0 || idx >= (int)P.t.size()) throw std::runtime_error("tensor index out of range");
    const Tn& t = P.t[idx];
    if (info4) { info4[0] = t.rows; info4[1] = t.C; info4[2] = t.ld; info4[3] = t.f32 ? 1 : 0; }
    if (!host_out) return DD_OK;
    // the gradient slab is packed by liveness: after a run only the pinned ranges (program inputs / outputs, padded tensors) still hold
    // the tensor's own gradient -- an intermediate's range may have been reused by another tensor since
    if (want_grad && t.grad && !(t.glo < 0 && t.ghi >= (int)P.ops.size()) && !E->sw.no_grad_reuse)
      throw std::runtime_error("gradient of an intermediate tensor: its range of the liveness-packed slab is reused during the reverse run "
                               "(build the engine with DD_NO_GRAD_REUSE=1 to read it)");
    HIPCHK(hipDeviceSynchronize());
    char* slab = E->inst[k].act[prog];
    if (!want_grad && !slab) throw std::runtime_error("this instance has no slab for that program");
    char* base = want_grad ? E->grad_slab + t.goff : t.transient ? E->tr_slab + (size_t)t.tr_slot * P.tr_max : slab + t.off;
    const size_t n = (size_t)t.rows * t.ld;
    if ((t.f32 && !want_grad) || (want_grad && t.gf32)) { HIPCHK(hipMemcpy(host_out, base, n * 4, hipMemcpyDeviceToHost)); }
    else {
      std::vector<bf16_t> tmp(n);
      HIPCHK(hipMemcpy(tmp.data(), base, n * 2, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < n; ++i) host_out[i] = host_bf2f(tmp[i]);
    }
  });
}
// parity-test hook: image DEVICE fp32 [B,3,8L,8L] (not denormalised) replaces the decoder's output in front of the bicubic resize of
// every later guided forward (the gradient still flows through the decoder); NULL switches it off.  The caller keeps the buffer alive.
int dd_debug_set_images(dd_engine* E, const float* images, int count) {
  if (!E || count < 0) return DD_ERR_ARG;
  E->image_override = count > 0 ? images : nullptr;
  E->image_override_count = E->image_override ? count : 0;
  return DD_OK;
}
int dd_debug_set_image(dd_engine* E, const float* image) { return dd_debug_set_images(E, image, 1); }
// the statistics fusions fixed at finalize, four ints per op (include/distdiff_hip_ops.h); prog 0 unet, 1 vae, 2 guide, 3 vae encoder
int dd_debug_fusion_plan(dd_engine* E, int prog, int* out, int cap) {
  if (!E || prog < 0 || prog > 3 || (cap > 0 && !out)) return DD_ERR_ARG;
  if (!E->finalized) { E->err = "finalize first"; return DD_ERR_STATE; }
  const Program& P = E->prog[prog];
  for (int i = 0; i < (int)P.ops.size() && i < cap; ++i) {
    const Op& op = P.ops[i];
    out[4 * i] = op.kind;
    out[4 * i + 1] = (op.kind == OP_CONV || op.kind == OP_GN) && op.part ? (int)op.gn_fused : -1;
    out[4 * i + 2] = (op.kind == OP_CONV && op.rowstat_emit) || (op.kind == OP_LN && op.ln_fold) ? op.row_spans : -1;
    out[4 * i + 3] = 0;
  }
  return (int)P.ops.size();
}
int dd_debug_num_tensors(dd_engine* E, int prog) {
  if (!E || prog < 0 || prog > 2) return DD_ERR_ARG;
  return (int)E->prog[prog].t.size();
}

// ---- the plans as data (tests/test_engine_plans.py; field order: include/distdiff_hip_ops.h) ----
int dd_debug_plan_only(dd_engine* E) {
  if (!E) return DD_ERR_ARG;
  if (E->finalized) { E->err = "dd_debug_plan_only after dd_finalize_weights"; return DD_ERR_STATE; }
  E->plan_only = true;
  return DD_OK;
}
int dd_debug_plan_dump(dd_engine* E, int prog, int64_t* out, int cap) {
  if (!E || prog < 0 || prog > dd_engine::NPROG || (cap > 0 && !out)) return DD_ERR_ARG;
  if (!E->finalized) { E->err = "finalize first"; return DD_ERR_STATE; }
  int n = 0;
  auto put = [&](auto... v) { ((n < cap ? (void)(out[n] = (int64_t)v) : (void)0, ++n), ...); };
  if (prog == dd_engine::NPROG) {      // the engine record
    put(E->total_bytes, E->partial_cap, E->tmp_cap, E->packed.size());
    for (auto& p : E->packed) put(p.second);
    return n;
  }
  const Program& P = E->prog[prog];
  auto index_of = [](const auto& owned, const void* p) {
    for (size_t i = 0; i < owned.size(); ++i) if (owned[i].get() == p) return (int)i;
    return -1;
  };
  put(P.t.size(), P.ops.size(), P.act_bytes, P.grad_bytes, P.scratch_partial, P.scratch_tmp, P.scratch_rowpart, P.tr_max, P.tr_count);
  for (const Tn& t : P.t) put(t.off, t.goff, t.parent, t.rows, t.C, t.ld, t.B, t.H, t.W, t.f32, t.grad, t.gf32, t.transient, t.tr_slot, t.glo, t.ghi);
  for (const Op& o : P.ops) {
    uint64_t h = 1469598103934665603ull;      // FNV-1a over the producer list
    for (int pi : o.producers) h = (h ^ (uint64_t)(uint32_t)pi) * 1099511628211ull;
    uint32_t eps; memcpy(&eps, &o.eps, 4);
    int64_t flops; memcpy(&flops, &o.flops, 8);
    put(o.kind, o.x, o.y, o.res, o.raw, o.q, o.k, o.v, o.x2, index_of(E->convs, o.cw), index_of(E->norms, o.nw), o.stride, o.up, o.relu, o.out_f32,
        o.use_table, o.G, o.silu, eps, o.heads, o.D, o.Nq, o.Nk, o.cross_slot, o.causal, o.act_kind, o.pv_fp8, o.q_prescaled, o.patch, o.sel_stride,
        o.stats_off, o.fused, o.x_acc, o.res_acc, o.x2_acc, o.res_alias, o.part, o.part_off, o.part_ld, o.producers.size(), h, o.gn_fused, o.ln_fold,
        o.x_fwd, o.ln_stats_off, o.rowstat_from, o.rowstat_emit, o.rowstat_ld, o.row_spans, flops);
  }
  return n;
}

// output stage (generate_data.py:1227-1234): [B,3,H,W] fp32 in [0,1] -> uint8 HWC with torchvision.save_image's quantisation
int dd_image_to_u8(dd_engine* E, const float* image, uint8_t* out_hwc, int B, void* stream) {
  if (!E || !image || !out_hwc || B < 1) return DD_ERR_ARG;
  DD_TRY(E, {
    const dd_config& c = E->cfg;
    HIPCHK(launch_to_uint8(image, out_hwc, B, c.vae_out_channels, 8 * c.latent_size, 8 * c.latent_size, (hipStream_t)stream));
  });
}

size_t dd_workspace_bytes(dd_engine* e) { return e ? e->total_bytes : 0; }
double dd_flops_last(dd_engine* e) { if (!e) return 0; const double f = e->flops; e->flops = 0; return f; }

}  // extern "C"
