// Execution of a Program: forward and hand-derived reverse runs over the op list (no autograd), op by op on the HIP kernels.
#include <cstdint>
#include <string>
#include "engine_internal.h"

namespace ddi {

// ---- execution ----
static void fill_conv(ConvGemmParams& p, const Ctx& c) {
  memset(&p, 0, sizeof p);
  p.partial = (float*)c.scratch_partial;
  p.alpha = 1.f;
}

// fp32 programs (the guide network): conv forward / dgrad on guide_f32.hip
static void conv_f32_geometry(ConvF32Params& p, const ConvW* w, bool bwd) {
  const PackedConv& sh = bwd ? w->sb : w->sf;
  p.w = bwd ? w->wf_bwd : w->wf_fwd; p.taptab = bwd ? w->tap_bwd : w->tap_fwd;
  p.cin = sh.cin; p.ntaps = sh.ntaps; p.N = sh.N; p.K = sh.K;
  p.groups = w->groups;
  const int gi = w->Cin / w->groups, go = w->Cout / w->groups;
  p.cpg_in = bwd ? go : gi; p.cpg_out = bwd ? gi : go;
}

static void run_conv_f32_fwd(const Program& P, const Op& op, const Ctx& c) {
  const Tn& x = P.t[op.x]; const Tn& y = P.t[op.y];
  const ConvW* w = op.cw;
  ConvF32Params p; memset(&p, 0, sizeof p);
  conv_f32_geometry(p, w, false);
  p.x = act_f32(c, x); p.x_ld = x.ld; p.y = act_f32(c, y); p.y_ld = y.ld;
  p.B = x.B; p.H = x.H; p.W = x.W; p.Ho = y.H; p.Wo = y.W; p.stride = op.stride; p.M = y.rows;
  if (w->bias) { p.flags |= CF_BIAS; p.bias = w->bias; }
  if (op.res >= 0) { p.flags |= CF_RES; p.res = act_f32(c, P.t[op.res]); p.res_ld = P.t[op.res].ld; }
  if (op.relu == 1) p.flags |= CF_RELU;
  if (op.relu == 2) p.flags |= CF_RELU6;
  HIPCHK(launch_conv_f32(p, c.s));
}

// forward launch parameters of a bf16 convolution / linear op (everything but the statistics fusions)
static void fwd_conv_params(const Program& P, const Op& op, const Ctx& c, ConvGemmParams& p) {
  const Tn& x = P.t[op.x_fwd >= 0 ? op.x_fwd : op.x]; const Tn& y = P.t[op.y];
  fill_conv(p, c);
  const ConvW* w = op.cw;
  p.x = act_ptr(c, x); p.x_ld = x.ld; p.w = w->w_fwd; p.taptab = w->tap_fwd;
  p.y = act_raw(c, y); p.y_ld = y.ld;
  p.B = x.B; p.H = x.H; p.W = x.W; p.Ho = y.H; p.Wo = y.W; p.stride = op.stride; p.shift = op.up; p.parity = 0;
  p.cin = w->sf.cin; p.ntaps = w->sf.ntaps; p.M = y.rows; p.N = w->sf.N; p.K = w->sf.K;
  int flags = 0;
  if (op.use_table && w->bias_table) { flags |= CF_BIAS; p.bias = w->bias_table + (size_t)c.step_index * w->Cout; }
  else if (w->bias) { flags |= CF_BIAS; p.bias = w->bias; }
  if (op.res >= 0) { flags |= CF_RES; p.res = act_ptr(c, P.t[op.res]); p.res_ld = P.t[op.res].ld; }
  if (op.relu) flags |= CF_RELU;
  if (op.out_f32) flags |= CF_OUT_F32;
  if (w->geglu) {
    flags |= CF_GEGLU;
    if (op.raw >= 0 && c.stash) { flags |= CF_GEGLU_RAW; p.raw = act_ptr(c, P.t[op.raw]); p.raw_ld = P.t[op.raw].ld; }
  }
  if (op.ln_fold) { flags |= CF_LNFOLD; p.ln_stats = (const float*)(c.act + op.ln_stats_off); p.ln_c1 = w->ln_c1; }
  p.flags = flags;
}

// launch parameters of an attention op, forward or backward (cross attention: K, V are the prompt's constants, no dk / dv)
static AttnParams attn_params(const Program& P, const Op& op, const Ctx& c, bool bwd) {
  const Tn& q = P.t[op.q]; const Tn& y = P.t[op.y];
  AttnParams p; memset(&p, 0, sizeof p);
  p.q = act_ptr(c, q); p.ldq = q.ld;
  if (op.cross_slot >= 0) {
    p.k = (*c.cross_kv)[op.cross_slot].first; p.v = (*c.cross_kv)[op.cross_slot].second; p.ldk = p.ldv = q.C;
  } else {
    const Tn& k = P.t[op.k]; const Tn& v = P.t[op.v];
    p.k = act_ptr(c, k); p.v = act_ptr(c, v); p.ldk = k.ld; p.ldv = v.ld;
    if (bwd) { p.dk = grad_ptr(c, k); p.dv = grad_ptr(c, v); p.lddk = k.ld; p.lddv = v.ld; }
  }
  p.o = act_ptr(c, y); p.ldo = y.ld; p.lse = (float*)(c.act + op.stats_off);
  p.B = q.B; p.H = op.heads; p.Nq = op.Nq; p.Nk = op.Nk; p.D = op.D; p.scale = op.q_prescaled ? 0.6931471805599453f : 1.f / sqrtf((float)op.D); p.q_prescaled = op.q_prescaled;
  if (bwd) {
    p.delta = p.lse + (size_t)q.B * op.heads * op.Nq;
    p.d_o = grad_ptr(c, y); p.lddo = y.ld; p.dq = grad_ptr(c, q); p.lddq = q.ld;
  } else {
    p.causal = op.causal;
    p.pv_fp8 = op.pv_fp8;      // BASELINE configs[4]: fp8 P.V for d = 64 heads (SDXL), opt-in per engine (dd_config.unet_attn_fp8)
  }
  return p;
}
// the wide-head GEMM route may use the engine's scratch for self attention only
static AttnScratch attn_scratch(const Op& op, const Ctx& c) {
  if (op.cross_slot >= 0) return AttnScratch{};
  return AttnScratch{c.scratch_tmp, c.tmp_cap, c.tap1x1, (float*)c.scratch_partial, c.partial_cap};
}

// SDXL text_time conditioning: the time-embedding bias of this conv differs per image, it runs as one launch per image
static bool per_image_bias(const Op& op, const Ctx& c) { return op.use_table && c.img_bias > 0; }

// What the launcher's planner grants the statistics epilogues of forward conv `op` on its launch parameters p (fwd_conv_params):
// GroupNorm partials (CF_STATS) yes / no, and the column spans of LayerNorm row partials (CF_ROWSTATS; 0 = none).  An op that is a
// candidate for both keeps CF_STATS: one statistics epilogue per launch.  A function of shapes, leading dimensions, flags, partial_cap
// and which pointers are null only, so the answer at finalize (resolve_fusions) is the answer at every launch.
struct Fusions { bool stats; int spans; };
static Fusions ask_fusions(const Program& P, const Op& op, const Ctx& c, ConvGemmParams p) {
  Fusions f{false, 0};
  if (op.rowstat_emit && !op.part && c.rowpart) {
    ConvGemmParams q = p;
    q.rowpart = c.rowpart; q.rowpart_ld = op.rowstat_ld;
    int spans = 0;
    if (conv_gemm_can_emit_rowstats(q, c.partial_cap, &spans) && spans <= op.rowstat_ld) f.spans = spans;
  }
  if (op.part) {
    const Tn& y = P.t[op.y];
    p.stats = (float*)(c.act + op.part_off); p.stats_ld = op.part_ld;
    bool whole = true;
    if (per_image_bias(op, c)) { p.B = 1; p.M = y.H * y.W; whole = !(p.M & 63); }      // an image's launch must fill whole 64-row blocks
    f.stats = whole && conv_gemm_can_emit_stats(p, c.partial_cap);
  }
  return f;
}

void resolve_fusions(Program& P, const Ctx& c) {
  int ngn = 0, nmerge = 0, nfold = 0, nrows = 0;
  for (Op& op : P.ops) {
    if (op.kind == OP_CONV && (op.part || op.rowstat_emit)) {
      ConvGemmParams p;
      fwd_conv_params(P, op, c, p);
      if (op.use_table) p.flags |= CF_BIAS;      // the bias tables arrive with dd_set_schedule
      const Fusions f = ask_fusions(P, op, c, p);
      op.gn_fused = f.stats; op.row_spans = f.spans;
    } else if (op.kind == OP_GN) {
      op.gn_fused = op.part;
      for (int pi : op.producers) op.gn_fused = op.gn_fused && P.ops[pi].gn_fused;
      ++ngn; nmerge += op.gn_fused;
    } else if (op.kind == OP_LN && op.ln_fold) {
      op.row_spans = op.rowstat_from >= 0 ? P.ops[op.rowstat_from].row_spans : 0;
      ++nfold; nrows += op.row_spans > 0;
    }
  }
  if (getenv("DD_PLAN_REPORT"))
    fprintf(stderr, "[plan] statistics fusions: %d of %d GroupNorms merge their producers' partials, %d of %d folded LayerNorms read row partials\n", nmerge, ngn, nrows, nfold);
}

static int op_family(const Program& P, const Op& op) {
  return (op.kind == OP_CONV && !P.f32) ? Profiler::CONV : op.kind == OP_ATTN ? Profiler::ATTN
         : (op.kind == OP_GN || op.kind == OP_LN) ? Profiler::NORM : Profiler::OTHER;
}
static double attn_bwd_flops(const Op& op) { return op.flops * (op.cross_slot >= 0 ? 1.5 : 2.5); }
// the profiler record of op's forward (bwd = 0) or backward (1) run: family, algorithmic flops and the GEMM / attention shape
static void prof_begin(const Program& P, const Op& op, const Ctx& c, int bwd) {
  if (!c.prof) return;
  const int fam = op_family(P, op);
  const PackedConv* g = op.kind != OP_CONV ? nullptr : bwd ? &op.cw->sb : &op.cw->sf;
  if (g) c.prof->begin(fam, op.flops, c.s, bwd ? P.t[op.x].rows << (2 * op.up) : P.t[op.y].rows, g->N, g->K, bwd);
  else if (op.kind == OP_ATTN) c.prof->begin(fam, bwd ? attn_bwd_flops(op) : op.flops, c.s, op.Nq, op.Nk, op.D, bwd);
  else c.prof->begin(fam, 0.0, c.s, P.t[op.x].rows, P.t[op.x].C, 0, bwd);
}
struct ProfEnd { const Ctx& c; ~ProfEnd() { if (c.prof) c.prof->end(c.s); } };      // also when the op throws
static void count_flops(const Ctx& c, double flops) { if (c.flops) *c.flops += flops; }

// ---- forward and backward: one function per op kind and direction, FWD / BWD in OpKind order ----
static void fwd_conv(const Program& P, const Op& op, const Ctx& c) {
  if (P.f32) { count_flops(c, op.flops); return run_conv_f32_fwd(P, op, c); }
  const Tn& x = P.t[op.x_fwd >= 0 ? op.x_fwd : op.x]; const Tn& y = P.t[op.y];
  const ConvW* w = op.cw;
  ConvGemmParams p;
  fwd_conv_params(P, op, c, p);
  if (g_plan_check && (op.part || op.rowstat_emit)) {
    const Fusions f = ask_fusions(P, op, c, p);
    if (f.stats != op.gn_fused || f.spans != op.row_spans)
      throw std::runtime_error("fusion plan violated: op " + std::to_string(&op - P.ops.data()) + " was planned with (CF_STATS " + std::to_string(op.gn_fused) +
                               ", row spans " + std::to_string(op.row_spans) + "), this launch is granted (" + std::to_string(f.stats) + ", " +
                               std::to_string(f.spans) + ")");
  }
  // the statistics fusions fixed at finalize (resolve_fusions): LayerNorm row partials for the op that follows, GroupNorm partials
  if (op.row_spans > 0) { p.flags |= CF_ROWSTATS; p.rowpart = c.rowpart; p.rowpart_ld = op.rowstat_ld; }
  if (op.gn_fused) { p.flags |= CF_STATS; p.stats = (float*)(c.act + op.part_off); p.stats_ld = op.part_ld; }
  count_flops(c, op.flops);
  if (!per_image_bias(op, c)) { HIPCHK(launch_conv_gemm(p, c.partial_cap, c.s)); return; }
  // one launch per image of the batch (H x W rows each; at 128x128 / 64x64 / 32x32 latents an image still fills the chip),
  // each with its own row of the bias table
  if (x.B != c.img_bias || op.stride != 1 || op.up || !w->bias_table_img) throw std::runtime_error("per-image bias: unexpected conv geometry");
  const size_t xrows = (size_t)x.H * x.W, yrows = (size_t)y.H * y.W;
  ConvGemmParams q = p;
  q.B = 1; q.M = (int)yrows;
  for (int bi = 0; bi < x.B; ++bi) {
    ConvGemmParams r = q;
    r.x = p.x + bi * xrows * x.ld;
    r.y = (char*)p.y + bi * yrows * y.ld * 2;
    r.bias = w->bias_table_img + ((size_t)c.step_index * c.img_bias + bi) * w->Cout;
    if (op.gn_fused) r.stats = q.stats + (size_t)bi * (yrows / 64) * op.part_ld * 2;
    HIPCHK(launch_conv_gemm(r, c.partial_cap, c.s));
  }
}
static void fwd_gn(const Program& P, const Op& op, const Ctx& c) {
  const Tn& x = P.t[op.x]; const Tn& y = P.t[op.y];
  GroupNormParams p; memset(&p, 0, sizeof p);
  if (op.gn_fused) p.chan_part = (const float*)(c.act + op.part_off);      // every producer emitted its partials
  p.part_ld = op.part_ld;
  p.x = act_ptr(c, x); p.x_ld = x.ld; p.y = act_ptr(c, y); p.y_ld = y.ld;
  p.gamma = op.nw->gamma; p.beta = op.nw->beta; p.stats = (float*)(c.act + op.stats_off); p.scratch = c.gn_scratch;
  p.B = x.B; p.HW = x.H * x.W; p.C = x.C; p.G = op.G; p.eps = op.eps; p.silu = op.silu;
  HIPCHK(launch_groupnorm_fwd(p, c.s));
}
static void fwd_ln(const Program& P, const Op& op, const Ctx& c) {
  const Tn& x = P.t[op.x]; const Tn& y = P.t[op.y];
  LayerNormParams p; memset(&p, 0, sizeof p);
  p.x = act_ptr(c, x); p.x_ld = x.ld; p.y = act_ptr(c, y); p.y_ld = y.ld;
  p.gamma = op.nw->gamma; p.beta = op.nw->beta; p.stats = (float*)(c.act + op.stats_off); p.M = x.rows; p.C = x.C; p.eps = op.eps;
  if (op.ln_fold) {
    // folded into the linear that follows: statistics only, from the producing GEMM's row partials when it emits them
    p.y = nullptr;
    if (op.row_spans > 0) { p.rowpart = c.rowpart; p.rowpart_ld = op.rowstat_ld; p.spans = op.row_spans; }
  }
  HIPCHK(launch_layernorm_fwd(p, c.s));
}
static void fwd_attn(const Program& P, const Op& op, const Ctx& c) {
  HIPCHK(launch_attention(attn_params(P, op, c, false), attn_scratch(op, c), false, c.s));
  count_flops(c, op.flops);
}
static void fwd_concat(const Program& P, const Op& op, const Ctx& c) {
  if (op.fused) return;
  const Tn& a = P.t[op.x]; const Tn& b = P.t[op.x2]; const Tn& y = P.t[op.y];
  HIPCHK(launch_copy_bf16(act_ptr(c, a), a.ld, act_ptr(c, y), y.ld, y.rows, a.C, c.s));
  HIPCHK(launch_copy_bf16(act_ptr(c, b), b.ld, act_ptr(c, y) + a.C, y.ld, y.rows, b.C, c.s));
}
static void fwd_maxpool(const Program& P, const Op& op, const Ctx& c) {
  const Tn& x = P.t[op.x]; const Tn& y = P.t[op.y];
  if (P.f32) HIPCHK(launch_maxpool3x3s2_f32(act_f32(c, x), act_f32(c, y), x.B, x.H, x.W, x.ld, c.s));
  else HIPCHK(launch_maxpool3x3s2(act_ptr(c, x), act_ptr(c, y), x.B, x.H, x.W, x.C, c.s));
}
static void fwd_act(const Program& P, const Op& op, const Ctx& c) {
  const Tn& x = P.t[op.x]; const Tn& y = P.t[op.y];
  HIPCHK(launch_act_bf16(act_ptr(c, x), x.ld, act_ptr(c, y), y.ld, x.rows, x.C, op.act_kind, c.s));
}
static void fwd_patchify(const Program& P, const Op& op, const Ctx& c) {
  const Tn& x = P.t[op.x]; const Tn& y = P.t[op.y];
  HIPCHK(launch_patchify(act_f32(c, x), x.ld, act_ptr(c, y), x.B, x.H, op.patch, x.C, c.s));
}
static void fwd_vitembed(const Program& P, const Op& op, const Ctx& c) {
  const Tn& x = P.t[op.x]; const Tn& y = P.t[op.y];
  HIPCHK(launch_vit_embed(act_ptr(c, x), x.ld, op.nw->gamma, op.nw->beta, act_ptr(c, y), y.ld, x.B, x.H, x.C, c.s));
}
static void fwd_select(const Program& P, const Op& op, const Ctx& c) {
  const Tn& x = P.t[op.x]; const Tn& y = P.t[op.y];
  HIPCHK(launch_select_rows(act_ptr(c, x), x.ld, act_ptr(c, y), y.ld, x.B, op.sel_stride, x.C, c.s));
}
static void fwd_dup(const Program& P, const Op& op, const Ctx& c) {
  const Tn& x = P.t[op.x]; const Tn& y = P.t[op.y];
  HIPCHK(launch_copy_bf16(act_ptr(c, x), x.ld, act_ptr(c, y), y.ld, x.rows, rup(x.C, 8), c.s));
  HIPCHK(launch_copy_bf16(act_ptr(c, x), x.ld, act_ptr(c, y) + (size_t)x.rows * y.ld, y.ld, x.rows, rup(x.C, 8), c.s));
}

typedef void (*OpFn)(const Program&, const Op&, const Ctx&);
static const OpFn FWD[] = {fwd_conv, fwd_gn, fwd_ln, fwd_attn, fwd_concat, fwd_maxpool, fwd_act, fwd_patchify, fwd_vitembed, fwd_select, fwd_dup};

void run_fwd(const Program& P, const Ctx& c) {
  if (c.prof) c.prof->new_run();
  for (const Op& op : P.ops) {
    prof_begin(P, op, c, 0);
    ProfEnd _end{c};
    FWD[op.kind](P, op, c);
  }
}

// DD_GRAD_CHECK=1 validates the finalize-time plans at run time: every gradient access of run_bwd against the interval plan_grad_memory
// packed the slab by, every statistics fusion of run_fwd (resolve_fusions) against what the planner grants that launch
bool ddi::g_plan_check = getenv("DD_GRAD_CHECK") != nullptr && atoi(getenv("DD_GRAD_CHECK")) != 0;
static thread_local int t_bwd_op = INT32_MIN;     // op whose backward is running (INT32_MIN: outside run_bwd)
void ddi::grad_access_check(const Tn& t) {
  if (t_bwd_op == INT32_MIN) return;
  if (t_bwd_op < t.glo || t_bwd_op > t.ghi)
    throw std::runtime_error("gradient plan violated: the backward of op " + std::to_string(t_bwd_op) + " touches a gradient that is only live in [" +
                             std::to_string(t.glo) + ", " + std::to_string(t.ghi) + "]");
}

// The two row formats of a gradient: 16-bit rows (bf16 / fp16 programs) and fp32 rows (the guide programs, guide_f32.hip), each with
// its pointers, the columns its kernels cover for a C-channel tensor and its add / copy / mask launchers
struct Rows16 {
  typedef bf16_t T;
  static constexpr auto add = launch_add_bf16; static constexpr auto copy = launch_copy_bf16;
  static T* grad(const Ctx& c, const Tn& t) { return grad_ptr(c, t); }
  static const T* act(const Ctx& c, const Tn& t) { return act_ptr(c, t); }
  static int cols(int C) { return C; }
  static hipError_t mask(T* g, int ld, const T* y, int ldy, int rows, int cols, int, hipStream_t s) { return launch_mask_bf16(g, ld, y, ldy, g, ld, rows, cols, s); }
};
struct RowsF32 {
  typedef float T;
  static constexpr auto add = launch_add_f32; static constexpr auto copy = launch_copy_f32;
  static T* grad(const Ctx& c, const Tn& t) { return grad_f32(c, t); }
  static const T* act(const Ctx& c, const Tn& t) { return act_f32(c, t); }
  static int cols(int C) { return rup(C, 4); }
  static hipError_t mask(T* g, int ld, const T* y, int ldy, int rows, int cols, int relu, hipStream_t s) { return launch_mask_f32(g, ld, y, ldy, g, ld, rows, cols, relu == 2 ? 6.f : 0.f, s); }
};

// One contribution src [dst.rows, cols] to the gradient of `dst` (a residual, a skip, a duplicated tensor): the first write copies,
// later ones add, and a gradient that IS src (Op::res_alias) needs nothing
template <class F>
static void grad_fanout(const Ctx& c, const typename F::T* src, int src_ld, const Tn& dst, int cols, bool accumulate, bool alias = false) {
  if (accumulate) HIPCHK(F::add(F::grad(c, dst), dst.ld, src, src_ld, F::grad(c, dst), dst.ld, dst.rows, cols, c.s));
  else if (!alias) HIPCHK(F::copy(src, src_ld, F::grad(c, dst), dst.ld, dst.rows, cols, c.s));
}
// y = act(conv(x) + res): the activation mask from the forward output on g(y) in place, then the residual fan-out; returns g(y)
template <class F>
static typename F::T* conv_bwd_prologue(const Program& P, const Op& op, const Ctx& c) {
  const Tn& y = P.t[op.y];
  typename F::T* gy = F::grad(c, y);
  if (op.relu) HIPCHK(F::mask(gy, y.ld, F::act(c, y), y.ld, y.rows, F::cols(y.C), op.relu, c.s));
  if (op.res >= 0 && P.t[op.res].grad) grad_fanout<F>(c, gy, y.ld, P.t[op.res], F::cols(P.t[op.res].C), op.res_acc, op.res_alias);
  return gy;
}
static void conv_f32_dgrad(const Program& P, const Op& op, const Ctx& c, const float* gy) {
  const Tn& x = P.t[op.x]; const Tn& y = P.t[op.y];
  ConvF32Params p; memset(&p, 0, sizeof p);
  conv_f32_geometry(p, op.cw, true);
  p.x = gy; p.x_ld = y.ld;
  p.B = y.B; p.H = y.H; p.W = y.W; p.Ho = x.H; p.Wo = x.W; p.M = x.rows; p.stride = 1;
  if (op.stride == 2) { p.shift = 1; p.parity = 1; }
  float* gx = grad_f32(c, x);
  p.y = gx; p.y_ld = x.ld;
  if (op.x_acc) { p.flags |= CF_RES; p.res = gx; p.res_ld = x.ld; }
  HIPCHK(launch_conv_f32(p, c.s));
}
static void conv_16_dgrad(const Program& P, const Op& op, const Ctx& c, const bf16_t* gy) {
  const Tn& x = P.t[op.x]; const Tn& y = P.t[op.y];
  const ConvW* w = op.cw;
  const bf16_t* gin = gy; int gin_ld = y.ld;
  char* tmp = c.scratch_tmp;
  if (w->geglu) {
    bf16_t* draw = (bf16_t*)tmp; tmp += rup_sz((size_t)y.rows * w->Cout * 2, 256);
    HIPCHK(launch_geglu_bwd(act_ptr(c, P.t[op.raw]), P.t[op.raw].ld, gy, y.ld, draw, w->Cout, y.rows, w->Cout / 2, c.s));
    gin = draw; gin_ld = w->Cout;
  }
  ConvGemmParams p; fill_conv(p, c);
  p.x = gin; p.x_ld = gin_ld; p.w = w->w_bwd; p.taptab = w->tap_bwd;
  p.B = y.B; p.H = y.H; p.W = y.W;
  p.cin = w->sb.cin; p.ntaps = w->sb.ntaps; p.N = w->sb.N; p.K = w->sb.K;
  p.stride = 1;
  if (op.stride == 2) { p.shift = 1; p.parity = 1; }
  const int Hl = x.H << op.up, Wl = x.W << op.up;
  p.Ho = Hl; p.Wo = Wl; p.M = x.B * Hl * Wl;
  bf16_t* gx = grad_ptr(c, x);
  if (op.up) {
    bf16_t* hi = (bf16_t*)tmp;
    const int ldh = rup(w->Cin, 8);
    p.y = hi; p.y_ld = ldh; p.flags = 0;
    HIPCHK(launch_conv_gemm(p, c.partial_cap, c.s));
    HIPCHK(launch_sumpool2x2(hi, ldh, gx, x.ld, x.B, x.H, x.W, rup(x.C, 8), op.x_acc ? 1 : 0, c.s));
  } else {
    p.y = gx; p.y_ld = x.ld; p.flags = 0;
    if (op.x_acc) { p.flags |= CF_RES; p.res = gx; p.res_ld = x.ld; }
    HIPCHK(launch_conv_gemm(p, c.partial_cap, c.s));
  }
}
static void bwd_conv(const Program& P, const Op& op, const Ctx& c) {
  const bool dgrad = P.t[op.x].grad;
  if (!dgrad && !(op.res >= 0 && P.t[op.res].grad)) return;
  // mask and residual fan-out in the program's row format, then the dgrad GEMM
  if (P.f32) { const float* gy = conv_bwd_prologue<RowsF32>(P, op, c); if (dgrad) conv_f32_dgrad(P, op, c, gy); }
  else { const bf16_t* gy = conv_bwd_prologue<Rows16>(P, op, c); if (dgrad) conv_16_dgrad(P, op, c, gy); }
  if (dgrad) count_flops(c, op.flops);
}
static void bwd_gn(const Program& P, const Op& op, const Ctx& c) {
  const Tn& x = P.t[op.x]; const Tn& y = P.t[op.y];
  if (!x.grad) return;
  GroupNormParams p; memset(&p, 0, sizeof p);
  p.x = act_ptr(c, x); p.x_ld = x.ld;
  p.gamma = op.nw->gamma; p.beta = op.nw->beta; p.stats = (float*)(c.act + op.stats_off); p.scratch = c.gn_scratch;
  p.B = x.B; p.HW = x.H * x.W; p.C = x.C; p.G = op.G; p.eps = op.eps; p.silu = op.silu;
  p.dy = grad_ptr(c, y); p.dy_ld = y.ld; p.dx = grad_ptr(c, x); p.dx_ld = x.ld; p.accumulate = op.x_acc;
  HIPCHK(launch_groupnorm_bwd(p, c.s));
}
static void bwd_ln(const Program& P, const Op& op, const Ctx& c) {
  const Tn& x = P.t[op.x]; const Tn& y = P.t[op.y];
  if (!x.grad) return;
  LayerNormParams p; memset(&p, 0, sizeof p);
  p.x = act_ptr(c, x); p.x_ld = x.ld; p.gamma = op.nw->gamma; p.beta = op.nw->beta;
  p.stats = (float*)(c.act + op.stats_off); p.M = x.rows; p.C = x.C; p.eps = op.eps;
  p.dy = grad_ptr(c, y); p.dy_ld = y.ld; p.dx = grad_ptr(c, x); p.dx_ld = x.ld; p.accumulate = op.x_acc;
  HIPCHK(launch_layernorm_bwd(p, c.s));
}
static void bwd_attn(const Program& P, const Op& op, const Ctx& c) {
  if (!P.t[op.q].grad) return;
  HIPCHK(launch_attention(attn_params(P, op, c, true), attn_scratch(op, c), true, c.s));
  count_flops(c, attn_bwd_flops(op));
}
static void bwd_concat(const Program& P, const Op& op, const Ctx& c) {
  if (op.fused) return;
  const Tn& a = P.t[op.x]; const Tn& b = P.t[op.x2]; const Tn& y = P.t[op.y];
  const bf16_t* gy = grad_ptr(c, y);
  if (a.grad) grad_fanout<Rows16>(c, gy, y.ld, a, a.C, op.x_acc);
  if (b.grad) grad_fanout<Rows16>(c, gy + a.C, y.ld, b, b.C, op.x2_acc);
}
static void bwd_maxpool(const Program& P, const Op& op, const Ctx& c) {
  const Tn& x = P.t[op.x]; const Tn& y = P.t[op.y];
  if (!x.grad) return;
  if (op.x_acc) throw std::runtime_error("maxpool backward accumulate unsupported");
  if (P.f32) HIPCHK(launch_maxpool3x3s2_bwd_f32(act_f32(c, x), grad_f32(c, y), grad_f32(c, x), x.B, x.H, x.W, x.ld, c.s));
  else HIPCHK(launch_maxpool3x3s2_bwd(act_ptr(c, x), grad_ptr(c, y), grad_ptr(c, x), x.B, x.H, x.W, x.C, c.s));
}
static void bwd_act(const Program& P, const Op& op, const Ctx& c) {
  const Tn& x = P.t[op.x]; const Tn& y = P.t[op.y];
  if (!x.grad) return;
  HIPCHK(launch_act_bwd_bf16(act_ptr(c, x), x.ld, grad_ptr(c, y), y.ld, grad_ptr(c, x), x.ld, x.rows, x.C, op.act_kind, op.x_acc ? 1 : 0, c.s));
}
static void bwd_patchify(const Program& P, const Op& op, const Ctx& c) {
  const Tn& x = P.t[op.x]; const Tn& y = P.t[op.y];
  if (!x.grad) return;
  if (op.x_acc || !x.gf32) throw std::runtime_error("patchify backward: the image gradient must be an fp32 first write");
  HIPCHK(launch_patchify_bwd(grad_ptr(c, y), grad_f32(c, x), x.ld, x.B, x.H, op.patch, x.C, c.s));
}
static void bwd_vitembed(const Program& P, const Op& op, const Ctx& c) {
  const Tn& x = P.t[op.x]; const Tn& y = P.t[op.y];
  if (!x.grad) return;
  if (op.x_acc) throw std::runtime_error("vit_embed backward accumulate unsupported");
  HIPCHK(launch_vit_embed_bwd(grad_ptr(c, y), y.ld, grad_ptr(c, x), x.ld, x.B, x.H, x.C, c.s));
}
static void bwd_select(const Program& P, const Op& op, const Ctx& c) {
  const Tn& x = P.t[op.x]; const Tn& y = P.t[op.y];
  if (!x.grad) return;
  HIPCHK(launch_select_rows_bwd(grad_ptr(c, y), y.ld, grad_ptr(c, x), x.ld, x.B, op.sel_stride, x.C, op.x_acc ? 1 : 0, c.s));
}
static void bwd_dup(const Program& P, const Op& op, const Ctx& c) {
  const Tn& x = P.t[op.x]; const Tn& y = P.t[op.y];
  if (!x.grad) return;
  const bf16_t* gy = grad_ptr(c, y);
  const bf16_t* hi = gy + (size_t)x.rows * y.ld;
  const int cols = rup(x.C, 8);
  if (op.x_acc) {      // both halves are contributions to a gradient that exists
    grad_fanout<Rows16>(c, gy, y.ld, x, cols, true);
    grad_fanout<Rows16>(c, hi, y.ld, x, cols, true);
  } else {             // the first write is their sum
    HIPCHK(launch_add_bf16(gy, y.ld, hi, y.ld, grad_ptr(c, x), x.ld, x.rows, cols, c.s));
  }
}

static const OpFn BWD[] = {bwd_conv, bwd_gn, bwd_ln, bwd_attn, bwd_concat, bwd_maxpool, bwd_act, bwd_patchify, bwd_vitembed, bwd_select, bwd_dup};

void run_bwd(const Program& P, const Ctx& c) {
  if (c.prof) c.prof->new_run();
  struct OpScope { ~OpScope() { t_bwd_op = INT32_MIN; } } _scope;
  for (int i = (int)P.ops.size() - 1; i >= 0; --i) {
    const Op& op = P.ops[i];
    t_bwd_op = i;
    prof_begin(P, op, c, 1);
    ProfEnd _end{c};
    BWD[op.kind](P, op, c);
  }
}

}  // namespace ddi
