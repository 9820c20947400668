// Tape executor + C ABI (include/dpb.h) of the MI355X pullback engine.
//
// A network is a tape of NHWC ops over numbered activation buffers.  Three passes run over a
// prefix of the tape:
//   primal  : batch B, keeps EVERY activation, GroupNorm statistic and attention matrix resident
//             in HBM (288 GB/GPU makes recomputation pointless).  x_t and t are fixed during a
//             power iteration, so this pass runs once per sample, not once per JVP/VJP as the
//             reference's autodiff does (src/utils/utils.py:766-797).
//   tangent : nt = B*k tangents pushed forward through the same kernels (linear ops: identical
//             GEMM with M scaled by k; nonlinear ops: closed-form tangent using the primal stash).
//   adjoint : nt cotangents pulled back in reverse tape order, input gradients only (no weight
//             gradients), fan-in handled by first-write/accumulate flags per buffer.
// Ops whose inputs do not depend on x (time-embedding MLP, text-conditioning K/V projections)
// are primal-only.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/dpb.h"
#include "kernels.h"

namespace dpb {

static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
const char* last_error() { return g_err; }
thread_local long launch_count = 0;   // common.h: DPB_LAUNCH counts here

static inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }
static inline int round8(int v) { return (v + 7) / 8 * 8; }

struct Buf {
  int rows = 0, C = 0, kind = 0, Cv = 0;   // Cv: valid (un-padded) channels
  bool is_const = true;      // independent of x
  size_t p_off = 0, t_off = 0, g_off = 0, g_off0 = 0;   // g_off0: planned cotangent storage (g_off may be swapped within an adjoint pass)
};

struct AttnPlan {            // per attention op, persisted from the primal pass
  int heads = 0, d = 0, Lq = 0, Lk = 0, Lqp = 0, Lkp = 0;
  bool causal = false;                             // text-encoder attention: query i sees keys <= i (materialised path only)
  bool kv_const = false, fused = false, cross = false;   // cross: constant K/V, one-launch tangent / adjoint (attn_cross_kernel)
  int oq = 0, ok = 0, ov = 0;                      // column offsets of q / k / v inside their buffers (fused QKV projection)
  size_t P = 0, PT = 0, KT = 0, VT = 0, QT = 0, stats = 0;   // offsets
  // Folded route of a text-conditioned layer (fold_route below): K and V are constants of the sample, so to_q -> attention -> to_out is two products,
  // z Gt^T with the softmax Jacobian as its epilogue (EPI_XATT) and w Fk^T (+ residual); the adjoint is the mirror image with F and Gk.
  bool fold_ok = false;                            // the tape has the shape the route needs (found at create)
  bool fold_live = false;                          // the last stashing primal built the operands below
  int q_op = -1, o_op = -1;                        // the to_q and to_out products around the op
  size_t Gt = 0, Gk = 0, F = 0, Fk = 0, Pf = 0;    // offsets: Gt, F [H 128][C]; Gk, Fk [C][H 80] (16 bit); Pf fp32 probabilities [Lq][H][80]
  const char* gA = nullptr;                        // adjoint pass: the cotangent of to_out's output as conv_adj(to_out) found it (the residual swap may rename it)
};

struct Op {
  dpb_op_desc d;
  bool is_const = true;
  int attn = -1;             // index into plans
  size_t pstats = 0, tstats = 0;   // GroupNorm stat slots (offsets)
  size_t aff = 0;            // modulated GroupNorm: its per-sample affine tables, gamma_b [maxB][C] then beta_b [maxB][C] (fp32; offset)
  int geglu_next = -1;       // CONV (FF-in): the GEGLU op that is the only consumer of its output (interleaved layout) -> fused tangent epilogue
  int geglu_prev = -1;       // CONV (FF-out): the GEGLU op that produces its input                                   -> fused adjoint epilogue
  int ln_next = -1;          // CONV: the LayerNorm op that reads its 320-wide output  -> tangent: product + LayerNorm tangent in one launch (EPI_LN_TAN)
  int ln_prev = -1;          // CONV: the LayerNorm op whose output is its only input -> adjoint: product + LayerNorm adjoint in one launch (EPI_LN_ADJ)
  int fold_plan = -1, fold_role = 0;   // CONV next to a text-conditioned attention op that can take the folded route: its plan; 1 = to_q, 2 = to_out
};

}  // namespace dpb

using namespace dpb;

struct dpb_engine {
  int dtype = DT_F32, es = 4;
  int maxB = 1, maxT = 1;
  std::vector<Buf> bufs;
  std::vector<Op> ops;
  std::vector<AttnPlan> plans;
  std::vector<int> producer;        // buffer -> op index producing it (-1 for inputs)
  std::vector<std::vector<int>> mod_users;   // op -> the modulated GroupNorm ops whose (scale, shift) its output holds: their affine tables are filled right after it
  int x_buf = -1, x_channels = 0, temb_buf = -1, temb_dim = 0, temb_flip = 0, temb_hm1 = 0, ctx_buf = -1;
  // Per-sample timesteps (dpb_primal_t): every SHARED buffer has max_batch rows, and the SHARED ops run once per sample into that sample's row.
  // That is sound only if nothing but a SHARED op or a row bias reads a SHARED buffer; empty: it is, else what stands against it (found at create).
  std::string per_sample_t_why;
  bool temb_read = false;           // some op reads temb_buf (an autoencoder or text-encoder tape only fills the slot: its output does not depend on t)
  hipStream_t stream = 0;
  char* ws = nullptr;
  size_t ws_bytes = 0;
  // arena offsets
  size_t pstats_off = 0, pstats_bytes = 0, tstats_off = 0, tstats_bytes = 0, gnpart = 0, gnpart_bytes = 0, gnticket = 0;
  size_t S1 = 0, S2 = 0, T1 = 0, Dv = 0, convtmp = 0, io_in = 0, io_out = 0, orth = 0, slab = 0, slab_bytes = 64u << 20, zeros = 0;
  size_t orth_stride = 0;                  // re-orthonormalisation scratch per sample of the batch
  size_t pbW = 0;                          // pullback loop fp32 staging of W = J^T J V
  size_t temb_host_stage = 0;
  int cur_batch = 0;
  std::vector<int> uses;            // buffer -> number of ops reading it (op_inputs)
  // A buffer (op) is ACTIVE for a seed -- x_buf for the encoder entry points, any buffer for the *_between ones -- if it is reachable forward from
  // it (an op: one of its differentiated inputs is); only active buffers carry tangents and cotangents.  For x_buf the flags are exactly
  // !is_const.  One flag vector per seed, computed on first use (seed_flags); a pass carries its seed's flags in its Pass.
  std::vector<std::vector<char>> act_cache;   // seed buffer -> [n_buffers + n_ops] flags (empty: not computed yet)
  int primal_last = -1;             // last op whose primal state (with the tangent / adjoint stash) is resident; -1: none
  // Scratch of the pass being run, kept here only because a pass must not allocate: every pass function resets the ones it uses at its start,
  // nothing in them is read across passes.  (What a pass depends on is in its Pass, what it reports in n_launch / flops / gbytes.)
  struct { bool on = false; GemmArgs a; } pend;   // a split-K product whose reduction is deferred to the normalisation op that consumes it
  std::vector<char> ginit;          // adjoint: buffers whose cotangent has been written (first write / accumulate)
  std::vector<char> skip;           // ops whose work a fused epilogue of another op has done in the current pass
  long n_launch = 0;                // dpb_engine_stats: the last pass's launches, GEMM flops and bytes
  double flops = 0, gbytes = 0;
  // captured power iteration (dpb_debug_set("graph_iterate", 1)), valid for one (tap, k, batch, buffer set)
  struct GraphKey {
    int tap, k, B; const void *V, *U, *s, *conv;
    bool operator==(const GraphKey& o) const { return tap == o.tap && k == o.k && B == o.B && V == o.V && U == o.U && s == o.s && conv == o.conv; }
  };
  hipGraphExec_t gexec = nullptr;
  GraphKey gkey{};
  long g_launches = 0; double g_flops = 0, g_bytes = 0;
  // optional per-launch timing of the GEMM kernel (bench.py roofline leg); off in the timed region
  bool profiling = false;
  struct Prof { hipEvent_t a, b; double flops; int big; int M, N, K, Z, gather; };
  std::vector<Prof> prof;
  float prof_overhead_ms = 0.f;     // elapsed time of an EMPTY event bracket on this stream (calibrated in dpb_engine_profile), subtracted per launch

  char* P(int b) const { return ws + bufs[b].p_off; }
  char* T(int b) const { return ws + bufs[b].t_off; }
  char* G(int b) const { return ws + bufs[b].g_off; }
};

namespace {

int fail(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return -1;
}

// What a primal pass is asked for beyond (x, t, ctx, upto): built by the entry point that means it, handed down by value.
struct Forward {
  bool stash = true;                // keep the tangent / adjoint stash (dpb_primal); false: forward only (dpb_forward, the DDIM loop)
  bool temb_resident = false;       // P(temb_buf) already holds this t's embedding (dpb_local_pca_sample, chunks after the first): no upload, no sync
  int seed = -1;                    // buffer replaced after its producer has run (-1: none), by ...
  const float* h = nullptr;         // ... the caller's activation (dpb_forward_from), or
  // ... P(seed)[g xbatch + b] <- P(seed)[b] + scale[.] * u[dir[.]] (dpb_forward_shift, dpb_forward_shift_groups): the batch is `groups` copies of
  // the xbatch samples of x / ctx, row g * xbatch + b is sample b in group g.  xbatch is the batch of ops 0 .. producer[seed]; groups > 1: the
  // shared prefix, the rest of the tape runs on copies
  const float* u = nullptr; const int32_t* dir = nullptr; const float* scale = nullptr;
  int xbatch = 0, groups = 0;
};

// Everything an op function may know about the pass it runs in.  Built on the stack by primal_pass / jvp_pass / vjp_pass.
struct Pass {
  int mode, tap;                    // MODE_*; the buffer the pass ends at (adjoint: starts from)
  int src;                          // seed buffer: x_buf for the encoder entry points and the primal pass, any buffer for the *_between ones
  const char *bact, *oact;          // [n_buffers], [n_ops] activity for that seed (seed_flags)
  Forward fwd;                      // primal only
  bool per_sample_t = false;        // primal only: the samples have timesteps of their own -- row b of every SHARED buffer is sample b's
  int srow = 0;                     // ... and the row the SHARED op being run reads and writes (0: the one row of a shared timestep)
  Pass(const dpb_engine* e, int mode_, int tap_, int src_, const char* flags)
      : mode(mode_), tap(tap_), src(src_), bact(flags), oact(flags + e->bufs.size()) {}
};

// The buffers an op reads: in0; in1 of ATTENTION and CONCAT; in2 of ATTENTION; res of CONV (when it has one); in1 of a modulated GROUPNORM (the
// SHARED embedding projection: read in the primal pass only, it carries no tangent).  An id its op kind does not read means nothing
// (include/dpb.h) and is never looked at.
struct OpInputs {
  int id[4], n;
  const int* begin() const { return id; }
  const int* end() const { return id + n; }
};
OpInputs op_inputs(const dpb_op_desc& d) {
  OpInputs r{{d.in0}, 1};
  if (d.kind == DPB_OP_ATTENTION || d.kind == DPB_OP_CONCAT) r.id[r.n++] = d.in1;
  if (d.kind == DPB_OP_ATTENTION) r.id[r.n++] = d.in2;
  if (d.kind == DPB_OP_CONV && d.res >= 0) r.id[r.n++] = d.res;
  if (d.kind == DPB_OP_GROUPNORM && d.ip[2]) r.id[r.n++] = d.in1;
  return r;
}
bool gn_modulated(const dpb_op_desc& d) { return d.kind == DPB_OP_GROUPNORM && d.ip[2] != 0; }

// the launches of one pass (dpb_engine_stats): what DPB_LAUNCH counted while the pass ran, on every way out of it
struct LaunchSpan {
  dpb_engine* e; long at;
  explicit LaunchSpan(dpb_engine* e_) : e(e_), at(launch_count) {}
  ~LaunchSpan() { e->n_launch = launch_count - at; }
};

// primal storage of a buffer as the op being run sees it: of a SHARED buffer, the row of the sample the op runs for
char* primal_ptr(const dpb_engine* e, const Pass& ps, int b) {
  const Buf& bf = e->bufs[b];
  return e->P(b) + (bf.kind == DPB_BUF_SHARED ? (size_t)ps.srow * bf.rows * bf.C * e->es : 0);
}

void gemm_prep(dpb_engine* e, GemmArgs& a) {
  a.slab = (float*)(e->ws + e->slab);
  a.zeros = e->ws + e->zeros;
  a.slab_bytes = e->slab_bytes;
}

// split-K products whose consumer is a GroupNorm (one-launch kernel) / LayerNorm leave their slabs to it (A/B switch: DPB_LAZY_REDUCE=0,
// dpb_debug_set("lazy_reduce", 0): every split-K product runs its own reduce kernel; the results are bitwise the same)
int g_lazy_reduce = getenv("DPB_LAZY_REDUCE") ? atoi(getenv("DPB_LAZY_REDUCE")) : 1;
// LayerNorm tangent / adjoint in the epilogue of the neighbouring 320-wide product (A/B switch: DPB_LN_FUSE=0, dpb_debug_set("ln_fuse", 0))
// Default OFF since round 6: with write-through output stores the separate product + ln_rows launches are 0.5 % ahead on the headline (118.4 / 118.5 vs 117.7 /
// 117.9 it/s, same session, profiles/r06_switch_ab.txt) and equal on the 80-tangent pass -- the row-complete 128 x 320 tile is one block per CU, and what it saved was
// mostly the dirty write-back of the intermediate at the kernel boundary.  The fused tile stays in the library (tests/test_gpu_edge.py) behind the switch.
int g_ln_fuse = getenv("DPB_LN_FUSE") ? atoi(getenv("DPB_LN_FUSE")) : 0;
int g_ln_kmax = getenv("DPB_LN_FUSE_KMAX") ? atoi(getenv("DPB_LN_FUSE_KMAX")) : 1024;   // adjoint: longest K that still takes the row-complete LayerNorm tile (tuning switch)

int flush_pending(dpb_engine* e) {                 // the designated consumer did not come next: reduce the parked product the ordinary way
  if (!e->pend.on) return 0;
  e->pend.on = false;
  return launch_gemm_reduce(e->dtype, e->pend.a, e->stream);
}

// ---- measurement brackets (dpb_engine_profile): an event pair around one launch (or one fused group of launches) with its algorithmic flops.
// kind: 0..6 the GEMM kernel kinds (include/dpb.h), 7 flash attention forward, 8 fused attention tangent, 9 fused attention adjoint (query-major +
// key-major launches together; `gather` holds the route bits of attn_adj_route_bits; for kind 8 it holds the kernel's waves per block), 10 one-launch
// cross-attention tangent / adjoint
int prof_open(dpb_engine* e, double flops, int kind, int M, int N, int K, int Z, int gather) {
  if (!e->profiling) return -1;
  dpb_engine::Prof p;
  p.flops = flops; p.big = kind; p.M = M; p.N = N; p.K = K; p.Z = Z; p.gather = gather;
  if (hipEventCreate(&p.a) != hipSuccess) return -1;
  if (hipEventCreate(&p.b) != hipSuccess) { (void)hipEventDestroy(p.a); return -1; }
  (void)hipEventRecord(p.a, e->stream);
  e->prof.push_back(p);
  return (int)e->prof.size() - 1;
}
void prof_close(dpb_engine* e, int idx) {
  if (idx >= 0) (void)hipEventRecord(e->prof[idx].b, e->stream);
}

// GEGLU in the epilogue of the forward pass's unsplit FF-in products (A/B switch: DPB_GEGLU_FWD=0, dpb_debug_set("geglu_fwd", 0))
int g_geglu_fwd = getenv("DPB_GEGLU_FWD") ? atoi(getenv("DPB_GEGLU_FWD")) : 1;
// one-launch forward of the text-conditioned attention layers (A/B switch: DPB_CROSS_PRIMAL=0, dpb_debug_set("cross_primal", 0): the materialised path)
int g_cross_primal = getenv("DPB_CROSS_PRIMAL") ? atoi(getenv("DPB_CROSS_PRIMAL")) : 1;
// Folded text-conditioned attention (A/B switch: DPB_CROSS_FOLD, dpb_debug_set("cross_fold", v)): 0 off; 1 the rule of fold_route; 2 wherever the tape
// allows it (tests at C = 320); v > 2: the rule, for layers of at least v channels (one level at a time)
int g_cross_fold = getenv("DPB_CROSS_FOLD") ? atoi(getenv("DPB_CROSS_FOLD")) : 1;
// THE route rule.  The layer is on the one-launch cross route with its to_q / to_out neighbours private to it (fold_ok, found at create); one sample
// (Gt, Gk, F, Fk are operands of the sample); and the folded products cost no more MACs per row than the chain they replace:
// (128 + 80) H C against 2 C^2 + 4 * 96 C.  SD-1.x (8 heads): C >= 640; SD-2.x (H = C / 64) and every C < 640: never.
bool fold_route(const dpb_engine* e, const AttnPlan& p) {
  if (!g_cross_fold || !p.fold_ok || e->cur_batch != 1 || !g_cross_primal) return false;
  if (g_cross_fold == 2) return true;
  const long H = p.heads, C = H * p.d;
  return 208 * H * C <= 2 * C * C + 384 * C && (g_cross_fold == 1 || C >= g_cross_fold);
}
// ... and whether a tangent / adjoint pass takes it: the operands are there and the pass runs the whole chain (seeded upstream of to_q, ending at
// or after to_out), so neither the q tangent nor the attention output is anybody's input or result
bool fold_on(const dpb_engine* e, const Pass& ps, const AttnPlan& p) {
  return p.fold_live && fold_route(e, p) && e->producer[ps.src] < p.q_op && e->producer[ps.tap] >= p.o_op;
}
int gemm(dpb_engine* e, GemmArgs a, bool can_defer = false) {
  // a product parked by an EARLIER gemm() of the same op (run_op has flushed everything older) must be reduced before this one reuses the slabs
  if (e->pend.on)
    if (int r = flush_pending(e)) return r;
  gemm_prep(e, a);
  GemmArgs* pend = (can_defer && g_lazy_reduce) ? &e->pend.a : nullptr;
  const double fl = 2.0 * a.M * (double)a.N * ((double)a.K + (a.A2 ? a.K2 : 0)) * a.Z1 * a.Z2;
  e->flops += fl;
  e->gbytes += ((double)a.M * a.K + (double)a.N * a.K + (double)a.M * a.N) * a.Z1 * a.Z2 * e->es;
  const GemmPlan pl = gemm_plan(e->dtype, a);   // the one dispatch of this launch: launch_gemm runs it, the bracket is labelled with its tile's profile kind
  // (-1 with profiling off) the same bracket helpers as the attention launches (an event that cannot be created or recorded costs the bracket, never leaks its partner)
  const int pi = prof_open(e, fl, pl.row ? pl.row->kind : 0, a.M, a.N, a.K, a.Z1 * a.Z2, a.gather);
  const int r = launch_gemm(e->dtype, a, e->stream, pend, &pl);
  e->pend.on = pend && pend->splitk > 1;
  prof_close(e, pi);
  return r;
}

// ------------------------------------------------------------------ CONV
// primal (n=B) or tangent (n=nt)
int conv_fwd(dpb_engine* e, const Op& op, const Pass& ps, int n) {
  const dpb_op_desc& d = op.d;
  const int mode = ps.mode;
  const int H = d.ip[0], W = d.ip[1], Cin = d.ip[2], Ho = d.ip[3], Wo = d.ip[4], Cout = d.ip[5], KS = d.ip[6];
  const Buf& bi = e->bufs[d.in0];
  const Buf& bo = e->bufs[d.out];
  if (mode == 1 && !ps.bact[d.in0]) {   // only the residual carries a tangent
    return launch_axpy(e->dtype, e->T(d.res), e->T(d.out), (long)n * bo.rows * bo.C, 0, e->stream);
  }
  GemmArgs g;
  const bool shared_out = bo.kind == DPB_BUF_SHARED;
  const int ns = shared_out ? 1 : n;
  g.A = mode == 0 ? primal_ptr(e, ps, d.in0) : e->T(d.in0);
  g.B = d.w[0];
  g.C = mode == 0 ? primal_ptr(e, ps, d.out) : e->T(d.out);
  g.N = Cout;
  g.K = KS * KS * Cin;
  g.ldb = g.K;
  g.ldc = bo.C;
  g.lda = bi.C;
  g.gather = d.ip[9];
  if (g.gather == GATHER_NONE) {
    g.M = ns * bi.rows;
  } else {
    g.M = ns * Ho * Wo;
    g.H = H; g.W = W; g.Cin = Cin; g.Ho = Ho; g.Wo = Wo; g.KS = KS; g.stride = d.ip[7]; g.pad = d.ip[8];
  }
  if (mode == 0) {
    g.bias = (const float*)d.w[2];
    if (d.rowbias >= 0) {
      g.rowbias = e->P(d.rowbias) + (size_t)d.ip[10] * e->es;      // ip[10]: column window of a net-wide fused projection (tape.py shared_begin)
      g.rows_per_sample = bo.rows;
      g.ldrb = e->bufs[d.rowbias].rows * e->bufs[d.rowbias].C;     // the pitch of the fused projection's rows, not this op's N
      g.rowbias_div = ps.per_sample_t ? 1 : 1 << 30;               // one row per sample, or row 0 for every sample
    }
  }
  if (d.res >= 0 && (mode == 0 || ps.bact[d.res])) {
    g.R = mode == 0 ? primal_ptr(e, ps, d.res) : e->T(d.res);
    g.ldr = e->bufs[d.res].C;
  }
  if (mode == 1 && op.fold_role && fold_on(e, ps, e->plans[op.fold_plan])) {
    const AttnPlan& p = e->plans[op.fold_plan];
    if (op.fold_role == 1) return 0;               // to_q: folded into Gt, the q tangent is never formed
    g.A = e->ws + e->S1; g.lda = 80 * p.heads;     // to_out: second folded product, w Fk^T (+ residual), K = 80 H
    g.B = e->ws + p.Fk; g.K = g.ldb = 80 * p.heads;
  }
  if (mode == 1 && op.ln_next >= 0 && g_ln_fuse) {   // the LayerNorm that reads this product's output: its tangent leaves the same launch
    const dpb_op_desc& ld = e->ops[op.ln_next].d;
    GemmArgs f = g;
    f.epi = EPI_LN_TAN; f.C2 = e->T(ld.out); f.ln_x = e->P(ld.in0); f.ln_gamma = (const float*)ld.w[0]; f.ln_eps = ld.fp[0];
    f.rows_per_sample = bo.rows; f.epi_kps = n / e->cur_batch;
    gemm_prep(e, f);
    if (gemm_epi_supported(e->dtype, f)) {
      e->skip[op.ln_next] = 1;
      return gemm(e, f);
    }
  }
  if (mode == 1 && op.geglu_next >= 0) {   // FF-in tangent: GEGLU's tangent in the epilogue, dh [rows][2F] is never written
    const dpb_op_desc& gd = e->ops[op.geglu_next].d;
    GemmArgs f = g;
    f.epi = EPI_GEGLU_TAN; f.hprim = e->P(d.out); f.epi_kps = n / e->cur_batch; f.rows_per_sample = bo.rows;
    f.C = e->T(gd.out); f.ldc = e->bufs[gd.out].C;
    gemm_prep(e, f);
    if (gemm_epi_supported(e->dtype, f)) {
      e->skip[op.geglu_next] = 1;
      return gemm(e, f);
    }
  }
  if (mode == 0 && !ps.fwd.stash && op.geglu_next >= 0 && g_geglu_fwd && !shared_out && d.out != ps.tap && d.out != ps.fwd.seed) {   // (a pass that stops AT h needs h written)
    // forward only (dpb_forward): an FF-in product that runs unsplit anyway applies GEGLU in its epilogue -- h [rows][2F] is neither written nor
    // re-read (84 MB per 64x64-level layer at batch 2), one launch less; bitwise the separate product + GEGLU kernel
    const dpb_op_desc& gd = e->ops[op.geglu_next].d;
    GemmArgs f = g;
    f.epi = EPI_GEGLU_FWD; f.C = e->P(gd.out); f.ldc = e->bufs[gd.out].C; f.rowbias = nullptr; f.R = nullptr;
    gemm_prep(e, f);
    GemmArgs probe = g; gemm_prep(e, probe);
    if (!g.rowbias && !g.R && gemm_epi_supported(e->dtype, f) && gemm_plan(e->dtype, probe).splitk == 1) {
      e->skip[op.geglu_next] = 1;
      return gemm(e, f);
    }
  }
  // tangent: a following one-launch GroupNorm / LayerNorm may add the split-K slabs itself.  (Primal / forward-only products too were tried in
  // round 3 -- bias and time-embedding row added by the consumer: 599 -> 573 launches per B = 2 forward but 7.47 -> 7.55 ms: the slabs are 16x
  // the bytes of the 16-bit tensor and the primal consumers have nothing to hide them under.)
  return gemm(e, g, mode == 1 && !shared_out);
}

int conv_adj(dpb_engine* e, const Op& op, const Pass& ps, int n) {
  const dpb_op_desc& d = op.d;
  const int H = d.ip[0], W = d.ip[1], Cin = d.ip[2], Ho = d.ip[3], Wo = d.ip[4], KS = d.ip[6];
  const Buf& bi = e->bufs[d.in0];
  const Buf& bo = e->bufs[d.out];
  const int Cout = bo.C;              // padded channel count of the cotangent (w[1] is [Cin][KS*KS*CoutPadded])
  if (ps.bact[d.in0]) {
    if (!d.w[1]) return fail("conv op has no transposed weight (w[1]) but its adjoint is needed");
    GemmArgs g;
    g.A = e->G(d.out);
    g.lda = bo.C;
    g.B = d.w[1];
    g.N = Cin;
    g.K = KS * KS * Cout;
    g.ldb = g.K;
    g.ldc = bi.C;
    const int gather = d.ip[9];
    if (op.fold_role && fold_on(e, ps, e->plans[op.fold_plan])) {
      AttnPlan& p = e->plans[op.fold_plan];
      if (op.fold_role == 2) {                     // to_out: folded into F -- attn_adjoint reads this op's cotangent itself; G(d.in0) stays unwritten
        p.gA = e->G(d.out);
        e->ginit[d.in0] = 1;
        goto residual;
      }
      g.A = e->ws + e->S1; g.lda = 80 * p.heads;   // to_q: second folded product, w Gk^T (the softmax scale is in Gk), K = 80 H
      g.B = e->ws + p.Gk; g.K = g.ldb = 80 * p.heads;
    }
    // the LayerNorm that wrote this product's input: its adjoint in the epilogue (K <= 1024: beyond -- the FF-in adjoint, K = 8 C -- the
    // row-complete tile's one block per CU loses more in the K loop than the fusion saves: g_ln_fuse bit 1 forces it for A/Bs)
    // (not when the input is the seed: the LayerNorm / GEGLU that wrote it is upstream of the pass, its cotangent G(seed) is the result)
    if (gather == GATHER_NONE && op.ln_prev >= 0 && g_ln_fuse && e->uses[d.in0] == 1 && d.in0 != ps.src && (g.K <= g_ln_kmax || (g_ln_fuse & 2))) {
      const dpb_op_desc& ld = e->ops[op.ln_prev].d;
      GemmArgs f = g;
      f.M = n * bi.rows;
      f.epi = EPI_LN_ADJ; f.C = e->G(ld.in0); f.ldc = e->bufs[ld.in0].C; f.accumulate = e->ginit[ld.in0];
      f.ln_x = e->P(ld.in0); f.ln_gamma = (const float*)ld.w[0]; f.ln_eps = ld.fp[0];
      f.rows_per_sample = bi.rows; f.epi_kps = n / e->cur_batch;
      gemm_prep(e, f);
      if (gemm_epi_supported(e->dtype, f)) {
        if (int r = gemm(e, f)) return r;
        e->ginit[ld.in0] = 1;               // G(d.in0) stays unwritten: the LayerNorm op sees ginit == 0 and is skipped
        goto residual;
      }
    }
    if (gather == GATHER_NONE && op.geglu_prev >= 0 && d.in0 != ps.src) {   // FF-out adjoint: GEGLU's adjoint in the epilogue, gy [rows][F] is never written
      const dpb_op_desc& gd = e->ops[op.geglu_prev].d;
      GemmArgs f = g;
      f.M = n * bi.rows;
      f.epi = EPI_GEGLU_ADJ; f.hprim = e->P(gd.in0); f.epi_kps = n / e->cur_batch; f.rows_per_sample = bi.rows;
      f.C = e->G(gd.in0); f.ldc = e->bufs[gd.in0].C; f.accumulate = e->ginit[gd.in0];
      gemm_prep(e, f);
      if (gemm_epi_supported(e->dtype, f)) {
        if (int r = gemm(e, f)) return r;
        e->ginit[gd.in0] = 1;               // G(d.in0) stays unwritten: the GEGLU op sees ginit == 0 and is skipped
        goto residual;
      }
    }
    const bool lone = e->uses[d.in0] == 1 && d.in0 != ps.src;     // the cotangent has this one contribution: its producer's adjoint may add the slabs
    if (gather == GATHER_NONE) {
      g.M = n * bi.rows;
      g.C = e->G(d.in0);
      g.accumulate = e->ginit[d.in0];
      if (int r = gemm(e, g, lone)) return r;
    } else if (gather == GATHER_CONV) {
      g.gather = GATHER_CONVT;
      g.M = n * H * W;
      g.H = Ho; g.W = Wo; g.Cin = Cout; g.Ho = H; g.Wo = W; g.KS = KS; g.stride = d.ip[7]; g.pad = d.ip[8];
      g.C = e->G(d.in0);
      g.accumulate = e->ginit[d.in0];
      if (int r = gemm(e, g, lone)) return r;
    } else {   // UPCONV: adjoint conv at the upsampled resolution, then 2x2 sum pooling
      g.gather = GATHER_CONVT;
      g.M = n * Ho * Wo;
      g.H = Ho; g.W = Wo; g.Cin = Cout; g.Ho = Ho; g.Wo = Wo; g.KS = KS; g.stride = 1; g.pad = 1;
      g.C = e->ws + e->convtmp;
      if (int r = gemm(e, g)) return r;
      if (int r = launch_pool2x2_sum(e->dtype, e->ws + e->convtmp, e->G(d.in0), n, H, W, bi.C, e->ginit[d.in0], e->stream)) return r;
    }
    e->ginit[d.in0] = 1;
  }
residual:
  if (d.res >= 0 && ps.bact[d.res]) {
    Buf& br = e->bufs[d.res];
    if (!e->ginit[d.res] && br.rows == bo.rows && br.C == bo.C && br.kind == bo.kind) {
      // first cotangent of the residual stream: G(out) is dead once its producer (this op) has run, so hand its storage
      // over instead of copying it (38 copies of up to 13 MB per adjoint pass on SD-1.5); dpb_vjp restores the plan
      std::swap(br.g_off, e->bufs[d.out].g_off);
    } else {
      if (int r = launch_axpy(e->dtype, e->G(d.out), e->G(d.res), (long)n * bo.rows * bo.C, e->ginit[d.res], e->stream)) return r;
    }
    e->ginit[d.res] = 1;
  }
  return 0;
}

// ------------------------------------------------------------------ norms / elementwise
// The normalisation op about to run reads `d`: if that is the output of the parked split-K product, hand it the slabs (run_op has already made
// sure that nothing else is parked).  `store`: the reduced tensor has other readers (residual stream, tap) and must be written as well.
void take_pending(dpb_engine* e, SlabSrc& src, const void* d, bool store) {
  if (!e->pend.on || e->pend.a.C != d) return;
  const GemmArgs& g = e->pend.a;
  src.slab = g.slab; src.splitk = g.splitk; src.MN = (long)g.M * g.N; src.N = g.N;
  src.R = g.R; src.ldr = g.ldr;
  src.store = store ? g.C : nullptr;
  e->pend.on = false;
}

// does `op`, about to run in `mode`, consume the parked product itself?  (GroupNorm: only the one-launch kernel takes slabs.)
bool consumes_pending(dpb_engine* e, const Op& op, int mode) {
  if (mode == MODE_PRIMAL || (op.d.kind != DPB_OP_GROUPNORM && op.d.kind != DPB_OP_LAYERNORM)) return false;
  const void* d = mode == MODE_TANGENT ? (const void*)e->T(op.d.in0) : (const void*)e->G(op.d.out);
  if (d != e->pend.a.C) return false;
  const Buf& bi = e->bufs[op.d.in0];
  if (e->pend.a.N != bi.C) return false;
  if (op.d.kind == DPB_OP_GROUPNORM) {
    GNArgs a; a.HW = bi.rows; a.C = bi.C; a.G = op.d.ip[0]; a.NT = 1;
    return groupnorm_is_one_launch(e->dtype, a);
  }
  return true;
}

// What GNArgs / LNArgs / GegluArgs share (same member names, kernels.h): the sample counts and, by mode, the input d, the output y and the
// first-write / accumulate flag of the cotangent
template <class A>
void fill_io(dpb_engine* e, const dpb_op_desc& d, const Pass& ps, int n, A& a) {
  if (ps.mode == MODE_PRIMAL) { a.Bp = n; a.y = e->P(d.out); return; }
  a.Bp = e->cur_batch; a.NT = n; a.kps = n / e->cur_batch;
  if (ps.mode == MODE_TANGENT) { a.d = e->T(d.in0); a.y = e->T(d.out); return; }
  a.d = e->G(d.out); a.y = e->G(d.in0);
  a.accumulate = e->ginit[d.in0];
  e->ginit[d.in0] = 1;
}
// ... and for the two normalisations, whose d may come from the parked product's slabs
template <class A>
void fill_norm_io(dpb_engine* e, const dpb_op_desc& d, const Pass& ps, int n, A& a) {
  fill_io(e, d, ps, n, a);
  if (ps.mode != MODE_PRIMAL) take_pending(e, a.src, a.d, ps.mode == MODE_TANGENT && (e->uses[d.in0] > 1 || d.in0 == ps.tap));
}

int gn_run(dpb_engine* e, const Op& op, const Pass& ps, int n) {
  const dpb_op_desc& d = op.d;
  const Buf& bi = e->bufs[d.in0];
  GNArgs a;
  a.x = e->P(d.in0);
  a.gamma = (const float*)d.w[0];
  a.beta = (const float*)d.w[1];
  if (gn_modulated(d)) {                           // scale-shift norm: sample b's affine (fill_affine, primal pass), in all three modes
    a.gamma = (const float*)(e->ws + op.aff);
    a.beta = a.gamma + (size_t)e->maxB * bi.C;
    a.astride = bi.C;
  }
  a.pstats = (double*)(e->ws + op.pstats);
  a.tstats = (double*)(e->ws + op.tstats);
  a.part = (float*)(e->ws + e->gnpart); a.part_bytes = e->gnpart_bytes; a.ticket = (int*)(e->ws + e->gnticket);
  a.det = gn_deterministic();
  a.HW = bi.rows; a.C = bi.C; a.G = d.ip[0]; a.silu = d.ip[1]; a.eps = d.fp[0];
  fill_norm_io(e, d, ps, n, a);
  return launch_groupnorm(e->dtype, ps.mode, a, e->stream);
}

int ln_run(dpb_engine* e, const Op& op, const Pass& ps, int n) {
  const dpb_op_desc& d = op.d;
  const Buf& bi = e->bufs[d.in0];
  LNArgs a;
  a.x = e->P(d.in0);
  a.gamma = (const float*)d.w[0];
  a.beta = (const float*)d.w[1];
  a.rows_per_sample = bi.rows; a.C = bi.C; a.eps = d.fp[0];
  fill_norm_io(e, d, ps, n, a);
  return launch_layernorm(e->dtype, ps.mode, a, e->stream);
}

int geglu_run(dpb_engine* e, const Op& op, const Pass& ps, int n) {
  const dpb_op_desc& d = op.d;
  const Buf& bi = e->bufs[d.in0];
  GegluArgs a;
  a.h = e->P(d.in0);
  a.rows_per_sample = bi.rows; a.F = bi.C / 2; a.il = d.ip[1];
  a.stash = ps.fwd.stash;
  fill_io(e, d, ps, n, a);
  return launch_geglu(e->dtype, ps.mode, a, e->stream);
}

// The affine tables of the modulated GroupNorm ops that read the output of op `src` (the fused embedding projection, just computed): rows
// 0 .. batch-1 -- the batch of the CALL, also when the projection itself ran in a shared prefix at batch 1 -- from row b of the projection when
// the samples have timesteps of their own, row 0 otherwise (the rule of a row bias: conv_fwd's rowbias_div).
int fill_affine(dpb_engine* e, int src, const Pass& ps, int batch) {
  const std::vector<int>& users = e->mod_users[src];
  if (users.empty()) return 0;
  const Buf& be = e->bufs[e->ops[src].d.out];
  std::vector<AdaGNOp> t(users.size());
  for (size_t i = 0; i < users.size(); ++i) {
    const Op& u = e->ops[users[i]];
    const int C = e->bufs[u.d.in0].C;
    t[i].gamma = (const float*)u.d.w[0]; t[i].beta = (const float*)u.d.w[1];
    t[i].emb = e->P(u.d.in1) + (size_t)u.d.ip[3] * e->es;
    t[i].og = (float*)(e->ws + u.aff); t[i].ob = t[i].og + (size_t)e->maxB * C;
    t[i].C = C;
  }
  return launch_adagn_affine(e->dtype, t.data(), (int)t.size(), (long)be.rows * be.C, batch, ps.per_sample_t ? 1 : 0, e->stream);
}

// 2x2 resampling (DPB_OP_RESAMPLE): primal and tangent are the map itself; the adjoint of the average pool is 0.25 x nearest upsampling, the
// adjoint of nearest upsampling the 2x2 sum, either added to what the cotangent of the input already holds (first write / accumulate)
int resample_run(dpb_engine* e, const Op& op, const Pass& ps, int n) {
  const dpb_op_desc& d = op.d;
  const bool up = d.ip[0] == 1;
  const int H = d.ip[1], W = d.ip[2], C = e->bufs[d.in0].C;
  const int h = up ? H : H / 2, w = up ? W : W / 2;            // the small side
  if (ps.mode == MODE_ADJOINT) {
    const int acc = e->ginit[d.in0];
    e->ginit[d.in0] = 1;
    return up ? launch_pool2x2(e->dtype, e->G(d.out), e->G(d.in0), n, h, w, C, 1.f, acc, e->stream)
              : launch_up2x2(e->dtype, e->G(d.out), e->G(d.in0), n, h, w, C, 0.25f, acc, e->stream);
  }
  const char* in = ps.mode == MODE_PRIMAL ? e->P(d.in0) : e->T(d.in0);
  char* out = ps.mode == MODE_PRIMAL ? e->P(d.out) : e->T(d.out);
  return up ? launch_up2x2(e->dtype, in, out, n, h, w, C, 1.f, 0, e->stream) : launch_pool2x2(e->dtype, in, out, n, h, w, C, 0.25f, 0, e->stream);
}

int concat_run(dpb_engine* e, const Op& op, const Pass& ps, int n) {
  const dpb_op_desc& d = op.d;
  const int mode = ps.mode;
  const Buf& b0 = e->bufs[d.in0];
  const Buf& b1 = e->bufs[d.in1];
  const Buf& bo = e->bufs[d.out];
  const long rows = (long)n * bo.rows;
  if (mode == MODE_ADJOINT) {
    if (ps.bact[d.in0]) {
      if (int r = launch_copy_cols(e->dtype, e->G(d.out), bo.C, 0, e->G(d.in0), b0.C, 0, rows, b0.C, e->ginit[d.in0], e->stream)) return r;
      e->ginit[d.in0] = 1;
    }
    if (ps.bact[d.in1]) {
      if (int r = launch_copy_cols(e->dtype, e->G(d.out), bo.C, b0.C, e->G(d.in1), b1.C, 0, rows, b1.C, e->ginit[d.in1], e->stream)) return r;
      e->ginit[d.in1] = 1;
    }
    return 0;
  }
  if (mode == MODE_TANGENT && (!ps.bact[d.in0] || !ps.bact[d.in1])) {
    // one operand does not depend on the seed (the skip half of an up-block concat when the pass starts at a tap): its window of the tangent
    // is zero -- written on every pass, since a pass of another seed may have left a tangent in that storage
    char* o = e->T(d.out);
    if (int r = ps.bact[d.in0] ? launch_copy_cols(e->dtype, e->T(d.in0), b0.C, 0, o, bo.C, 0, rows, b0.C, 0, e->stream)
                               : launch_zero_cols(e->dtype, o, bo.C, 0, rows, b0.C, e->stream)) return r;
    return ps.bact[d.in1] ? launch_copy_cols(e->dtype, e->T(d.in1), b1.C, 0, o, bo.C, b0.C, rows, b1.C, 0, e->stream)
                          : launch_zero_cols(e->dtype, o, bo.C, b0.C, rows, b1.C, e->stream);
  }
  char* o = mode == MODE_PRIMAL ? e->P(d.out) : e->T(d.out);
  const char* i0 = mode == MODE_PRIMAL ? e->P(d.in0) : e->T(d.in0);
  const char* i1 = mode == MODE_PRIMAL ? e->P(d.in1) : e->T(d.in1);
  if (int r = launch_copy_cols(e->dtype, i0, b0.C, 0, o, bo.C, 0, rows, b0.C, 0, e->stream)) return r;
  return launch_copy_cols(e->dtype, i1, b1.C, 0, o, bo.C, b0.C, rows, b1.C, 0, e->stream);
}

// ------------------------------------------------------------------ attention (materialised scores)
// Operand addressing: q / k / v may be column windows of wider buffers (fused QKV projection: one [rows][3C] buffer),
// so every operand has its own row stride (ld*) and column offset (o*); the output buffer is [rows][C].
struct AttnPtrs {
  const char *Q, *K, *V; char* O;
  int ldq, ldk, ldv, ldo;
};
static AttnPtrs attn_ptrs(dpb_engine* e, const dpb_op_desc& d, const AttnPlan& p, int which /*0 primal, 1 tangent, 2 cotangent*/) {
  AttnPtrs a;
  auto base = [&](int b) { return which == 0 ? e->P(b) : which == 1 ? e->T(b) : e->G(b); };
  a.ldq = e->bufs[d.in0].C; a.ldk = e->bufs[d.in1].C; a.ldv = e->bufs[d.in2].C; a.ldo = e->bufs[d.out].C;
  a.Q = base(d.in0) + (size_t)p.oq * e->es;
  a.K = (which == 0 || !p.kv_const) ? base(d.in1) + (size_t)p.ok * e->es : nullptr;
  a.V = (which == 0 || !p.kv_const) ? base(d.in2) + (size_t)p.ov * e->es : nullptr;
  a.O = base(d.out);
  return a;
}

void fill_fused(dpb_engine* e, const AttnPlan& p, const AttnPtrs& x, FusedAttnArgs& f, int kps, float scale) {
  char* ws = e->ws;
  f.Q = x.Q; f.K = x.K; f.V = x.V; f.O = x.O; f.VT = ws + p.VT; f.KT = ws + p.KT; f.QT = ws + p.QT;
  f.stats = (const float*)(ws + p.stats);
  f.L = p.Lq; f.C = x.ldq; f.Co = x.ldo; f.H = p.heads; f.d = p.d; f.kps = kps; f.scale = scale; f.fl = e->dtype == DT_F16;
}
// one-launch constant-K/V attention: Y [..][Cy] from X [..][Cx] (and BT, the per-head transpose the pass needs) on the primal q, k, v
void fill_cross(dpb_engine* e, const AttnPlan& p, const AttnPtrs& x, CrossAttnArgs& f, int kps, float scale, const void* BT, const void* X, int Cx,
                void* Y, int Cy) {
  f.Q = x.Q; f.K = x.K; f.V = x.V; f.BT = BT; f.X = X; f.Y = Y;
  f.L = p.Lq; f.Lk = p.Lk; f.Lkp = p.Lkp; f.C = x.ldq; f.Ck = x.ldk; f.Cx = Cx; f.Cy = Cy;
  f.H = p.heads; f.d = p.d; f.kps = kps; f.scale = scale; f.fl = e->dtype == DT_F16;
}

// one attention launch with its flops (n_prod L x L x d products per sample or tangent and head) counted and its measurement bracket around it
template <class F>
int attn_launch(dpb_engine* e, const AttnPlan& p, int kind, int n_prod, int Z1, int gather, F launch) {
  const double fl = 2.0 * p.Lq * (double)p.Lk * p.d * n_prod * Z1 * p.heads;
  e->flops += fl;
  const int pi = prof_open(e, fl, kind, p.Lq, p.Lk, p.d, Z1 * p.heads, gather);
  const int r = launch();
  prof_close(e, pi);
  return r;
}

// The operands of the materialised path's batched products (z1: sample or tangent, z2: head) have one of two per-head layouts:
//   rows: head h is the column window [h d, (h + 1) d) of a [L][ld] row buffer   -> sample stride L ld, head stride d
//   tile: head h is a dense [rows][Lp] tile of a [Z][H][rows][Lp] scratch tensor -> sample stride H rows Lp, head stride rows Lp
// div: the operand is a primal one, shared by the `div` tangents of a sample.
enum Side { SIDE_A, SIDE_B, SIDE_C, SIDE_A2, SIDE_B2 };
void set_side(GemmArgs& g, Side s, const void* ptr, int ld, long s1, long s2, int div) {
  switch (s) {
    case SIDE_A: g.A = ptr; g.lda = ld; g.sA1 = s1; g.sA2 = s2; g.divA = div; break;
    case SIDE_B: g.B = ptr; g.ldb = ld; g.sB1 = s1; g.sB2 = s2; g.divB = div; break;
    case SIDE_C: g.C = (void*)ptr; g.ldc = ld; g.sC1 = s1; g.sC2 = s2; break;
    case SIDE_A2: g.A2 = ptr; g.lda2 = ld; g.sA21 = s1; g.sA22 = s2; g.divA2 = div; break;
    case SIDE_B2: g.B2 = ptr; g.ldb2 = ld; g.sB21 = s1; g.sB22 = s2; g.divB2 = div; break;
  }
}
void side_rows(GemmArgs& g, Side s, const void* ptr, int ld, int L, int d, int div = 1) { set_side(g, s, ptr, ld, (long)L * ld, d, div); }
void side_tile(GemmArgs& g, Side s, const void* ptr, int H, int rows, int Lp, int div = 1) {
  set_side(g, s, ptr, Lp, (long)H * rows * Lp, (long)rows * Lp, div);
}
void dims(GemmArgs& g, int M, int N, int K, int Z1, int Z2, float alpha = 1.f) { g.M = M; g.N = N; g.K = K; g.Z1 = Z1; g.Z2 = Z2; g.alpha = alpha; }
// rows layout [Z][L][ld] -> per-head transposes [Z][H][d][Lp] (zero padded)
int head_transpose(dpb_engine* e, const AttnPlan& p, const void* in, int ld, void* out, int Z, int L, int Lp) {
  return launch_transpose(e->dtype, in, out, Z, p.heads, (long)L * ld, p.d, L, p.d, ld, Lp, (long)p.d * Lp, e->stream);
}

// The operands of the folded route for the one sample of the pass, from its K, V (primal, 77 live rows) and the two weights; four batched products
// over the heads, fp32 accumulation, one rounding each.  The pad rows 77..127 of a head window of Gt / F and the pad columns 77..79 of Gk / Fk are
// never written: they are the zeros dpb_engine_set_workspace left (and EPI_XATT does not look at what a pad row produced).
//   Gt[h][j][c] = Gk[c][80 h + j] = scale K_h[j] . Wq[h d .., c]      F[h][j][c] = Fk[c][80 h + j] = V_h[j] . Wo[c, h d ..]
int fold_build(dpb_engine* e, const AttnPlan& p, const AttnPtrs& x, float scale) {
  const int H = p.heads, C = H * p.d, W = 80 * H;
  const void* WqT = e->ops[p.q_op].d.w[1];         // [C][C]: row = input channel, column = q channel
  const void* Wo = e->ops[p.o_op].d.w[0];          // [C][C]: row = output channel, column = attention channel
  char* ws = e->ws;
  for (int which = 0; which < 2; ++which) {
    const void* kv = which ? x.V : x.K; const int ldkv = which ? x.ldv : x.ldk;
    const void* w = which ? Wo : WqT;
    const float alpha = which ? 1.f : scale;
    GemmArgs t;                                    // key-major: [H 128][C]
    side_rows(t, SIDE_A, kv, ldkv, p.Lk, p.d);
    side_rows(t, SIDE_B, w, C, C, p.d);
    set_side(t, SIDE_C, ws + (which ? p.F : p.Gt), C, 0, 128L * C, 1);
    dims(t, p.Lk, C, p.d, 1, H, alpha);
    if (int r = gemm(e, t)) return r;
    GemmArgs k;                                    // channel-major: [C][80 H]
    side_rows(k, SIDE_A, w, C, C, p.d);
    side_rows(k, SIDE_B, kv, ldkv, p.Lk, p.d);
    set_side(k, SIDE_C, ws + (which ? p.Fk : p.Gk), W, 0, 80, 1);
    dims(k, C, p.Lk, p.d, 1, H, alpha);
    if (int r = gemm(e, k)) return r;
  }
  return 0;
}

// first folded product of a pass: X [nt rows][C] against the key-major operand B, softmax Jacobian in the epilogue -> e->S1 [nt rows][80 H]
int fold_product1(dpb_engine* e, const AttnPlan& p, const void* X, int ldx, size_t B, int nt) {
  const int H = p.heads, C = H * p.d;
  GemmArgs g;
  g.A = X; g.lda = ldx; g.B = e->ws + B; g.ldb = C;
  g.C = e->ws + e->S1; g.ldc = 80 * H;
  g.M = nt * p.Lq; g.N = 128 * H; g.K = C;
  g.epi = EPI_XATT; g.xatt_p = (const float*)(e->ws + p.Pf); g.xatt_h = H; g.xatt_lk = p.Lk;
  g.rows_per_sample = p.Lq; g.epi_kps = nt / e->cur_batch;
  return gemm(e, g);
}

int attn_primal(dpb_engine* e, const Op& op, const Pass& ps, int B) {
  const dpb_op_desc& d = op.d;
  const AttnPlan& p = e->plans[op.attn];
  const int H = p.heads;
  const bool stash = ps.fwd.stash;
  const float scale = 1.f / sqrtf((float)p.d);
  char* ws = e->ws;
  const AttnPtrs x = attn_ptrs(e, d, p, 0);
  if (p.fused) {   // flash forward: O and the row statistics, no L x L object; the kernels build transposed operand fragments with
                   // LDS transpose reads from the row tiles, so no per-head transposed copies are kept either
    FusedAttnArgs f;
    fill_fused(e, p, x, f, 1, scale);
    return attn_launch(e, p, 7, 2, B, 0, [&] { return launch_attn_fwd_fused(f, B, x.O, (float*)(ws + p.stats), e->stream); });
  }
  if (p.cross && g_cross_primal) {
    // text-conditioned layers: O = softmax(scale Q K^T) V in ONE launch (the 77 keys fit one masked tile; V^T is built in LDS), instead of
    // GEMM + softmax + transpose + GEMM; the tangent / adjoint kernels of the pullback passes still read the per-head V^T / K^T copies
    CrossAttnArgs f;
    fill_cross(e, p, x, f, 1, scale, nullptr, nullptr, x.ldq, x.O, x.ldo);
    f.primal = 1;
    // the folded route's stash, when the pass keeps one and runs the whole chain: the fp32 probabilities from this launch, the operands after it
    const bool fold = stash && fold_route(e, p) && e->producer[ps.tap] >= p.o_op;
    if (fold) f.Pstash = (float*)(ws + p.Pf);
    const int r = attn_launch(e, p, 10, 2, B, 2, [&] { return launch_attn_cross(f, B, e->stream); });
    if (r || !stash) return r;
    // (the head transposes stay: the one-launch route runs on the same stash when the switch is flipped between passes)
    if (int r2 = head_transpose(e, p, x.V, x.ldv, ws + p.VT, B, p.Lk, p.Lkp)) return r2;
    if (int r2 = head_transpose(e, p, x.K, x.ldk, ws + p.KT, B, p.Lk, p.Lkp)) return r2;
    if (fold) {
      if (int r2 = fold_build(e, p, x, scale)) return r2;
      e->plans[op.attn].fold_live = true;
    }
    return 0;
  }
  GemmArgs g;   // S = scale * Q K^T
  side_rows(g, SIDE_A, x.Q, x.ldq, p.Lq, p.d);
  side_rows(g, SIDE_B, x.K, x.ldk, p.Lk, p.d);
  side_tile(g, SIDE_C, ws + p.P, H, p.Lq, p.Lkp);
  dims(g, p.Lq, p.Lk, p.d, B, H, scale);
  if (int r = gemm(e, g)) return r;
  if (int r = launch_softmax_fwd(e->dtype, ws + p.P, (long)B * H, p.Lq, p.Lk, p.Lkp, p.causal, e->stream)) return r;
  // V^T, K^T per head ([d][Lkp], zero padded)
  if (int r = head_transpose(e, p, x.V, x.ldv, ws + p.VT, B, p.Lk, p.Lkp)) return r;
  if (stash)                        // K^T serves the adjoint only
    if (int r = head_transpose(e, p, x.K, x.ldk, ws + p.KT, B, p.Lk, p.Lkp)) return r;
  GemmArgs o;   // O = P V
  side_tile(o, SIDE_A, ws + p.P, H, p.Lq, p.Lkp);
  side_tile(o, SIDE_B, ws + p.VT, H, p.d, p.Lkp);
  side_rows(o, SIDE_C, x.O, x.ldo, p.Lq, p.d);
  dims(o, p.Lq, p.d, p.Lkp, B, H);
  if (int r = gemm(e, o)) return r;
  if (!p.kv_const && stash) {
    if (int r = launch_transpose(e->dtype, ws + p.P, ws + p.PT, B * H, 1, (long)p.Lq * p.Lkp, 0, p.Lq, p.Lk, p.Lkp, p.Lqp, (long)p.Lk * p.Lqp, e->stream)) return r;
    if (int r = head_transpose(e, p, x.Q, x.ldq, ws + p.QT, B, p.Lq, p.Lqp)) return r;
  }
  return 0;
}

int attn_tangent(dpb_engine* e, const Op& op, const Pass& ps, int nt) {
  const dpb_op_desc& d = op.d;
  const AttnPlan& p = e->plans[op.attn];
  const int H = p.heads, kps = nt / e->cur_batch;
  const float scale = 1.f / sqrtf((float)p.d);
  char* ws = e->ws;
  char* S1 = ws + e->S1;
  const AttnPtrs x = attn_ptrs(e, d, p, 0), t = attn_ptrs(e, d, p, 1);
  if (p.fused) {
    FusedAttnArgs f;
    fill_fused(e, p, x, f, kps, scale);
    f.dQ = t.Q; f.dK = t.K; f.dV = t.V; f.dO = t.O;
    // dS (2 products), dP V, P dV + the recomputed scores: 5 L x L x d products
    return attn_launch(e, p, 8, 5, nt, attn_jvp_block_waves(p.d, p.Lq, nt * H), [&] { return launch_attn_jvp_fused(f, nt, e->stream); });
  }
  if (p.cross && fold_on(e, ps, p)) {   // folded: w = P o (z Gt^T - delta), to_q skipped before, to_out multiplies by Fk after
    const int zb = e->ops[p.q_op].d.in0;
    return fold_product1(e, p, e->T(zb), e->bufs[zb].C, p.Gt, nt);
  }
  if (p.cross) {   // constant K/V: dO = [P o (scale dQ K^T - delta)] V in one launch
    CrossAttnArgs f;
    fill_cross(e, p, x, f, kps, scale, ws + p.VT, t.Q, t.ldq, t.O, t.ldo);
    return attn_launch(e, p, 10, 2, nt, 0, [&] { return launch_attn_cross(f, nt, e->stream); });
  }
  GemmArgs g;   // dS = scale * dQ K^T
  side_rows(g, SIDE_A, t.Q, t.ldq, p.Lq, p.d);
  side_rows(g, SIDE_B, x.K, x.ldk, p.Lk, p.d, kps);
  side_tile(g, SIDE_C, S1, H, p.Lq, p.Lkp);
  dims(g, p.Lq, p.Lk, p.d, nt, H, scale);
  if (!p.kv_const) {   // + scale * Q dK^T in the same launch (second operand pair)
    side_rows(g, SIDE_A2, x.Q, x.ldq, p.Lq, p.d, kps);
    side_rows(g, SIDE_B2, t.K, t.ldk, p.Lk, p.d);
    g.K2 = p.d;
  }
  if (int r = gemm(e, g)) return r;
  if (int r = launch_softmax_jvp(e->dtype, ws + p.P, S1, nullptr, (long)nt * H, H, kps, p.Lq, p.Lk, p.Lkp, e->stream)) return r;
  GemmArgs o;   // dO = dP V
  side_tile(o, SIDE_A, S1, H, p.Lq, p.Lkp);
  side_tile(o, SIDE_B, ws + p.VT, H, p.d, p.Lkp, kps);
  side_rows(o, SIDE_C, t.O, t.ldo, p.Lq, p.d);
  dims(o, p.Lq, p.d, p.Lkp, nt, H);
  if (!p.kv_const) {   // + P dV in the same launch
    char* T1 = ws + e->T1;
    if (int r = head_transpose(e, p, t.V, t.ldv, T1, nt, p.Lk, p.Lkp)) return r;
    side_tile(o, SIDE_A2, ws + p.P, H, p.Lq, p.Lkp, kps);
    side_tile(o, SIDE_B2, T1, H, p.d, p.Lkp);
    o.K2 = p.Lkp;
  }
  return gemm(e, o);
}

int attn_adjoint(dpb_engine* e, const Op& op, const Pass& ps, int nt) {
  const dpb_op_desc& d = op.d;
  const AttnPlan& p = e->plans[op.attn];
  const int H = p.heads, kps = nt / e->cur_batch;
  const float scale = 1.f / sqrtf((float)p.d);
  char* ws = e->ws;
  char* S1 = ws + e->S1;
  float* Dv = (float*)(ws + e->Dv);
  const AttnPtrs x = attn_ptrs(e, d, p, 0), c = attn_ptrs(e, d, p, 2);
  const char* gO = c.O;
  // first-write / accumulate flags, read up front: q, k, v may be windows of ONE buffer (fused QKV).  A window that IS an earlier-written one
  // (q, k and v of one [rows][C] input) accumulates onto it: gQ is written first; gV, then gK on the materialised path; the fused key-major
  // kernels write gK + gV once when their windows coincide
  const bool kq = d.in1 == d.in0 && p.ok == p.oq, vq = d.in2 == d.in0 && p.ov == p.oq, vk = d.in2 == d.in1 && p.ov == p.ok;
  const int accQ = e->ginit[d.in0], accK = p.kv_const ? 0 : e->ginit[d.in1] || kq || (!p.fused && vk),
            accV = p.kv_const ? 0 : e->ginit[d.in2] || vq;
  if (p.fused) {
    FusedAttnArgs f;
    fill_fused(e, p, x, f, kps, scale);
    f.gO = gO; f.gQ = (void*)c.Q; f.gK = (void*)c.K; f.gV = (void*)c.V; f.Drow = Dv;
    f.accQ = accQ; f.accK = accK; f.accV = accV;
    // query-major: scores, gP, gQ (3); key-major: scores^T, gP^T, gV, gK (4)
    if (int r = attn_launch(e, p, 9, 7, nt, attn_adj_route_bits(p.d, p.Lq, kps, nt), [&] { return launch_attn_adj_fused(f, nt, e->stream); })) return r;
    e->ginit[d.in0] = e->ginit[d.in1] = e->ginit[d.in2] = 1;
    return 0;
  }
  if (p.cross && fold_on(e, ps, p)) {   // folded: w = P o (g F^T - delta) from to_out's cotangent; to_q's adjoint multiplies by Gk (G(q) stays unwritten)
    if (int r = fold_product1(e, p, p.gA, e->bufs[e->ops[p.o_op].d.out].C, p.F, nt)) return r;
    e->ginit[d.in0] = 1;
    return 0;
  }
  if (p.cross) {   // constant K/V: gQ (+)= scale [P o (gO V^T - delta)] K in one launch
    CrossAttnArgs f;
    fill_cross(e, p, x, f, kps, scale, ws + p.KT, gO, c.ldo, (void*)c.Q, c.ldq);
    f.adjoint = 1; f.accumulate = accQ;
    if (int r = attn_launch(e, p, 10, 2, nt, 1, [&] { return launch_attn_cross(f, nt, e->stream); })) return r;
    e->ginit[d.in0] = 1;
    return 0;
  }
  GemmArgs g;   // gP = gO V^T
  side_rows(g, SIDE_A, gO, c.ldo, p.Lq, p.d);
  side_rows(g, SIDE_B, x.V, x.ldv, p.Lk, p.d, kps);
  side_tile(g, SIDE_C, S1, H, p.Lq, p.Lkp);
  dims(g, p.Lq, p.Lk, p.d, nt, H);
  if (int r = gemm(e, g)) return r;
  if (int r = launch_softmax_jvp(e->dtype, ws + p.P, S1, p.kv_const ? nullptr : Dv, (long)nt * H, H, kps, p.Lq, p.Lk, p.Lkp, e->stream)) return r;
  GemmArgs q;   // gQ (+)= scale * gS K
  side_tile(q, SIDE_A, S1, H, p.Lq, p.Lkp);
  side_tile(q, SIDE_B, ws + p.KT, H, p.d, p.Lkp, kps);
  side_rows(q, SIDE_C, c.Q, c.ldq, p.Lq, p.d);
  dims(q, p.Lq, p.d, p.Lkp, nt, H, scale);
  q.accumulate = accQ;
  if (int r = gemm(e, q)) return r;
  e->ginit[d.in0] = 1;
  if (p.kv_const) return 0;
  char* T1 = ws + e->T1;
  char* S2 = ws + e->S2;
  // gO^T per head [d][Lqp]
  if (int r = head_transpose(e, p, gO, c.ldo, T1, nt, p.Lq, p.Lqp)) return r;
  GemmArgs v;   // gV (+)= P^T gO
  side_tile(v, SIDE_A, ws + p.PT, H, p.Lk, p.Lqp, kps);
  side_tile(v, SIDE_B, T1, H, p.d, p.Lqp);
  side_rows(v, SIDE_C, c.V, c.ldv, p.Lk, p.d);
  dims(v, p.Lk, p.d, p.Lqp, nt, H);
  v.accumulate = accV;
  if (int r = gemm(e, v)) return r;
  GemmArgs t;   // gP^T = V gO^T
  side_rows(t, SIDE_A, x.V, x.ldv, p.Lk, p.d, kps);
  side_rows(t, SIDE_B, gO, c.ldo, p.Lq, p.d);
  side_tile(t, SIDE_C, S2, H, p.Lk, p.Lqp);
  dims(t, p.Lk, p.Lq, p.d, nt, H);
  if (int r = gemm(e, t)) return r;
  if (int r = launch_softmax_adjT(e->dtype, ws + p.PT, S2, Dv, (long)nt * H, H, kps, p.Lk, p.Lq, p.Lqp, e->stream)) return r;
  GemmArgs k;   // gK (+)= scale * gS^T Q
  side_tile(k, SIDE_A, S2, H, p.Lk, p.Lqp);
  side_tile(k, SIDE_B, ws + p.QT, H, p.d, p.Lqp, kps);
  side_rows(k, SIDE_C, c.K, c.ldk, p.Lk, p.d);
  dims(k, p.Lk, p.d, p.Lqp, nt, H, scale);
  k.accumulate = accK;
  if (int r = gemm(e, k)) return r;
  e->ginit[d.in1] = e->ginit[d.in2] = 1;
  return 0;
}

int run_op(dpb_engine* e, const Op& op, const Pass& ps, int n) {
  const int mode = ps.mode;
  if (e->pend.on && !consumes_pending(e, op, mode))
    if (int r = flush_pending(e)) return r;
  switch (op.d.kind) {
    case DPB_OP_CONV: return mode == MODE_ADJOINT ? conv_adj(e, op, ps, n) : conv_fwd(e, op, ps, n);
    case DPB_OP_GROUPNORM: return gn_run(e, op, ps, n);
    case DPB_OP_LAYERNORM: return ln_run(e, op, ps, n);
    case DPB_OP_GEGLU: return geglu_run(e, op, ps, n);
    case DPB_OP_CONCAT: return concat_run(e, op, ps, n);
    case DPB_OP_RESAMPLE: return resample_run(e, op, ps, n);
    case DPB_OP_ATTENTION:
      return mode == MODE_PRIMAL ? attn_primal(e, op, ps, n) : mode == MODE_TANGENT ? attn_tangent(e, op, ps, n) : attn_adjoint(e, op, ps, n);
    case DPB_OP_SILU: {
      if (mode != MODE_PRIMAL) return fail("SILU / quick-GELU ops are primal only (time-embedding path, text encoder)");
      const Buf& b = e->bufs[op.d.in0];
      const auto act = op.d.ip[0] == 2 ? launch_gelu : op.d.ip[0] == 1 ? launch_quick_gelu : launch_silu;
      return act(e->dtype, primal_ptr(e, ps, op.d.in0), primal_ptr(e, ps, op.d.out), (long)(b.kind == DPB_BUF_SHARED ? 1 : n) * b.rows * b.C, e->stream);
    }
  }
  return fail("unknown op kind %d", op.d.kind);
}

int check_tap(dpb_engine* e, int tap, int nt) {
  if (!e->ws) return fail("workspace not set (dpb_engine_set_workspace)");
  if (tap < 0 || tap >= (int)e->bufs.size() || e->producer[tap] < 0) return fail("invalid tap buffer %d", tap);
  if (e->bufs[tap].is_const) return fail("tap buffer %d does not depend on x", tap);
  if (e->cur_batch <= 0) return fail("dpb_primal must run before jvp/vjp");
  if (nt <= 0 || nt > e->maxT || nt % e->cur_batch) return fail("nt=%d must be a positive multiple of batch=%d and <= max_tangents=%d", nt, e->cur_batch, e->maxT);
  return 0;
}

// the activity flags of seed `src` ([n_buffers] buffers, then [n_ops] ops), computed once per seed and cached; nullptr (and the error set) if
// the tape cannot be differentiated from src.  Changes nothing but the cache.
const char* seed_flags(dpb_engine* e, int src) {
  const int nb = (int)e->bufs.size(), no = (int)e->ops.size();
  std::vector<char>& a = e->act_cache[src];
  if (!a.empty()) return a.data();
  std::vector<char> f(nb + no, 0);
  if (src == e->x_buf) {                          // the create-time flags, unchanged
    for (int b = 0; b < nb; ++b) f[b] = !e->bufs[b].is_const;
    for (int i = 0; i < no; ++i) f[nb + i] = !e->ops[i].is_const;
  } else {
    f[src] = 1;
    for (int i = e->producer[src] + 1; i < no; ++i) {   // ops up to producer[src] cannot read a buffer written later (SSA tape order)
      const Op& op = e->ops[i];
      const dpb_op_desc& d = op.d;
      bool on = false;
      for (int b : op_inputs(d)) on = on || f[b];
      if (d.kind == DPB_OP_SILU && on) { fail("op %d (SILU / GELU, primal only) depends on source buffer %d", i, src); return nullptr; }
      if (on && d.kind == DPB_OP_ATTENTION) {   // the attention kernels were planned for x: the query and (k, v) must have the same activity as for x
        const AttnPlan& p = e->plans[op.attn];
        if (!f[d.in0] || f[d.in1] != f[d.in2] || (bool)f[d.in1] == p.kv_const) {
          fail("attention op %d: q, k, v depend on source buffer %d differently than on x (unsupported)", i, src);
          return nullptr;
        }
      }
      f[nb + i] = on;
      if (on) f[d.out] = 1;
    }
  }
  a.swap(f);
  return a.data();
}

// channels of the seed's fp32 NCHW boundary: the network input's true channels, a tap's valid channels
int seed_channels(const dpb_engine* e, int src) { return src == e->x_buf ? e->x_channels : e->bufs[src].Cv; }

// The one validation of a (src, dst) pair; *flags: the seed's activity.  src must be an x-dependent activation an op produced, dst an op's
// output downstream of it.  pass: a tangent / adjoint pass -- x_buf is a seed too (the encoder Jacobian), and between two inner buffers the
// primal state must reach dst; otherwise a forward seeded at src (dpb_forward_from / _shift), which computes its own.
enum PairUse { FOR_FORWARD, FOR_PASS };
int check_pair(dpb_engine* e, int src, int dst, PairUse use, const char** flags = nullptr) {
  const int nb = (int)e->bufs.size();
  const bool pass = use == FOR_PASS, inner = !(pass && src == e->x_buf);
  if (inner) {
    if (src < 0 || src >= nb || e->producer[src] < 0 || e->bufs[src].kind != DPB_BUF_ACT) return fail("invalid source buffer %d (an activation produced by an op)", src);
    if (e->bufs[src].is_const) return fail("invalid source buffer %d: it does not depend on x", src);
  }
  if (dst < 0 || dst >= nb || e->producer[dst] < 0) return fail("invalid dst buffer %d", dst);
  if (pass && inner && e->producer[dst] > e->primal_last)
    return fail("no primal state up to dst buffer %d (produced by op %d, the primal pass covers ops 0..%d): run dpb_primal with upto_buf = dst or later",
                dst, e->producer[dst], e->primal_last);
  const char* f = seed_flags(e, src);
  if (!f) return -1;
  if (dst == src || !f[dst]) return fail("dst buffer %d is not downstream of source buffer %d", dst, src);
  if (flags) *flags = f;
  return 0;
}

// the checks of a tangent / adjoint pass from src to tap with nt directions
int check_pass(dpb_engine* e, int src, int tap, int nt, const char** flags = nullptr) {
  if (int r = check_tap(e, tap, nt)) return r;
  return check_pair(e, src, tap, FOR_PASS, flags);
}

}  // namespace

// =================================================================== C ABI
extern "C" {

const char* dpb_last_error(void) { return g_err; }
int dpb_abi_version(void) { return DPB_ABI_VERSION; }

int dpb_engine_create(const dpb_net_desc* net, dpb_engine** out) {
  if (!net || !out) return fail("null argument");
  if (net->dtype != DPB_F32 && net->dtype != DPB_BF16 && net->dtype != DPB_F16) return fail("bad dtype %d", net->dtype);
  if (net->max_batch < 1 || net->max_tangents < 1) return fail("max_batch/max_tangents must be >= 1");
  dpb_engine* e = new dpb_engine();
  e->dtype = net->dtype;
  e->es = net->dtype == DPB_F32 ? 4 : 2;
  e->maxB = net->max_batch;
  e->maxT = net->max_tangents;
  e->x_buf = net->x_buf; e->x_channels = net->x_channels; e->temb_buf = net->temb_buf; e->temb_dim = net->temb_dim;
  e->temb_flip = net->temb_flip_sin_to_cos; e->temb_hm1 = net->temb_half_minus_one; e->ctx_buf = net->ctx_buf;
  const int nb = net->n_buffers;
  e->bufs.resize(nb);
  e->producer.assign(nb, -1);
  auto bad = [&](const char* m, int i) { fail("op %d: %s", i, m); delete e; return -1; };
  for (int i = 0; i < nb; ++i) {
    e->bufs[i].rows = net->buffers[i].rows;
    e->bufs[i].C = net->buffers[i].channels;
    e->bufs[i].kind = net->buffers[i].kind;
    e->bufs[i].Cv = net->buffers[i].valid_channels > 0 ? net->buffers[i].valid_channels : net->buffers[i].channels;
    if (e->bufs[i].rows < 1 || e->bufs[i].C < 8 || e->bufs[i].C % 8) { fail("buffer %d: rows=%d channels=%d (channels must be a multiple of 8)", i, e->bufs[i].rows, e->bufs[i].C); delete e; return -1; }
  }
  if (net->x_buf < 0 || net->x_buf >= nb) { fail("bad x_buf"); delete e; return -1; }
  e->bufs[net->x_buf].is_const = false;
  auto okb = [&](int b) { return b >= 0 && b < nb; };
  for (int i = 0; i < net->n_ops; ++i) {
    Op op;
    op.d = net->ops[i];
    const dpb_op_desc& d = op.d;
    if (!okb(d.out)) return bad("bad buffer id", i);
    bool c = true;                                 // the output depends on x if any buffer the op reads does
    for (int b : op_inputs(d)) {
      if (!okb(b)) return bad("bad buffer id", i);
      c = c && e->bufs[b].is_const;
    }
    if (d.kind == DPB_OP_ATTENTION) {
      AttnPlan p;
      p.heads = d.ip[0];
      p.oq = d.ip[1]; p.ok = d.ip[2]; p.ov = d.ip[3];
      p.causal = d.ip[4] != 0;
      const int Cattn = e->bufs[d.out].C;
      if (p.heads < 1 || Cattn % p.heads) return bad("channels not divisible by heads", i);
      p.d = Cattn / p.heads;
      if (p.oq % 8 || p.ok % 8 || p.ov % 8 || p.oq + Cattn > e->bufs[d.in0].C || p.ok + Cattn > e->bufs[d.in1].C || p.ov + Cattn > e->bufs[d.in2].C)
        return bad("bad q/k/v column window", i);
      auto part = [&](int b0, int o0, int b1, int o1) { return b0 == b1 && o0 != o1 && o0 < o1 + Cattn && o1 < o0 + Cattn; };
      if (part(d.in0, p.oq, d.in1, p.ok) || part(d.in0, p.oq, d.in2, p.ov) || part(d.in1, p.ok, d.in2, p.ov))
        return bad("q/k/v windows of one buffer must coincide or be disjoint", i);
      if (p.d % 8) return bad("head dim must be a multiple of 8", i);
      p.Lq = e->bufs[d.in0].rows; p.Lk = e->bufs[d.in1].rows;
      p.Lqp = round8(p.Lq); p.Lkp = round8(p.Lk);
      if (e->bufs[d.in1].is_const != e->bufs[d.in2].is_const) return bad("k and v must both depend on x or both not", i);
      if (e->bufs[d.in0].is_const) return bad("attention query independent of x is unsupported", i);
      p.kv_const = e->bufs[d.in1].is_const;
      op.attn = (int)e->plans.size();
      e->plans.push_back(p);
    }
    if (d.kind == DPB_OP_CONV) {
      if (d.rowbias >= 0 && (!okb(d.rowbias) || e->bufs[d.rowbias].kind != DPB_BUF_SHARED)) return bad("rowbias must be a SHARED buffer", i);
      if (d.rowbias >= 0 && (d.ip[10] < 0 || d.ip[10] % 8 || d.ip[10] + round8(d.ip[5]) > e->bufs[d.rowbias].C)) return bad("bad rowbias column window", i);
      if (!d.w[0]) return bad("missing weight", i);
      if (d.ip[2] != e->bufs[d.in0].C || e->bufs[d.out].C != round8(d.ip[5])) return bad("conv channel mismatch", i);
    }
    if (d.kind == DPB_OP_GROUPNORM) {
      const Buf& gi = e->bufs[d.in0];
      if (gn_modulated(d)) {
        if (e->bufs[d.in1].kind != DPB_BUF_SHARED || e->bufs[d.in1].rows != 1 || e->producer[d.in1] < 0)
          return bad("modulated groupnorm: in1 must be a one-row SHARED buffer produced by an earlier op (the embedding projection)", i);
        if (gi.kind != DPB_BUF_ACT) return bad("modulated groupnorm: the normalised buffer must be a per-sample activation", i);
        if (d.ip[3] < 0 || d.ip[3] % 8 || d.ip[3] + 2 * gi.C > e->bufs[d.in1].C) return bad("modulated groupnorm: bad (scale | shift) column window", i);
        if (!d.w[0] || !d.w[1]) return bad("modulated groupnorm: missing gamma / beta", i);
      }
    }
    if (d.kind == DPB_OP_RESAMPLE) {
      const Buf& ri = e->bufs[d.in0];
      const Buf& ro = e->bufs[d.out];
      const int H = d.ip[1], W = d.ip[2];
      if (d.ip[0] != 0 && d.ip[0] != 1) return bad("resample: ip[0] must be 0 (2x2 average pool) or 1 (nearest x2 upsample)", i);
      if (H < 1 || W < 1 || (long)H * W != ri.rows || ri.C != ro.C || ri.kind != DPB_BUF_ACT || ro.kind != DPB_BUF_ACT) return bad("resample: input shape mismatch", i);
      if (d.ip[0] == 0 ? (H % 2 || W % 2 || (long)(H / 2) * (W / 2) != ro.rows) : (long)4 * H * W != ro.rows) return bad("resample: output shape mismatch", i);
    }
    for (int b : op_inputs(d)) e->temb_read = e->temb_read || b == e->temb_buf;
    if (e->per_sample_t_why.empty()) {              // per-sample timesteps: SHARED buffers are read by SHARED ops and as row biases only
      char why[160] = "";
      const bool so = e->bufs[d.out].kind == DPB_BUF_SHARED;
      for (int b : op_inputs(d))
        if ((e->bufs[b].kind == DPB_BUF_SHARED) != so && !(gn_modulated(d) && b == d.in1))   // (a modulated GroupNorm reads its sample's row through the affine tables)
          snprintf(why, sizeof(why), "op %d reads %s buffer %d into %s buffer %d", i, so ? "per-sample" : "SHARED", b, so ? "SHARED" : "per-sample", d.out);
      if (so && !(d.kind == DPB_OP_SILU || (d.kind == DPB_OP_CONV && d.ip[9] == DPB_GATHER_NONE && d.rowbias < 0)))
        snprintf(why, sizeof(why), "op %d writes SHARED buffer %d and is neither a linear layer nor an activation", i, d.out);
      e->per_sample_t_why = why;
    }
    op.is_const = c;
    e->bufs[d.out].is_const = c;
    if (e->producer[d.out] >= 0) return bad("buffer written twice (tape must be SSA)", i);
    e->producer[d.out] = i;
    e->ops.push_back(op);
  }
  e->mod_users.assign(e->ops.size(), std::vector<int>());
  for (size_t i = 0; i < e->ops.size(); ++i)
    if (gn_modulated(e->ops[i].d)) e->mod_users[e->producer[e->ops[i].d.in1]].push_back((int)i);
  // ---------------- GEGLU fusion pairs: FF-in conv -> GEGLU (interleaved layout, sole consumer) -> FF-out conv (sole consumer)
  {
    std::vector<int> uses(nb, 0), user(nb, -1);
    for (size_t i = 0; i < e->ops.size(); ++i) {
      for (int b : op_inputs(e->ops[i].d)) { uses[b]++; user[b] = (int)i; }
    }
    e->uses = uses;
    // LayerNorm fused into the neighbouring product's epilogue (row-complete 128 x 320 ring tile, 16-bit engines): tangent -- the product that
    // WRITES the LayerNorm input also writes the LayerNorm tangent; adjoint -- the adjoint of the product that READS the LayerNorm output
    // applies the LayerNorm adjoint to its result.  (The 64 x 64 level of SD: C = 320.)
    for (size_t j = 0; j < e->ops.size(); ++j) {
      const dpb_op_desc& d = e->ops[j].d;
      if (d.kind != DPB_OP_LAYERNORM || e->ops[j].is_const || e->dtype == DT_F32 || e->bufs[d.in0].C != 320 || e->bufs[d.in0].kind != DPB_BUF_ACT) continue;
      const int pi = e->producer[d.in0];
      if (pi >= 0 && e->ops[pi].d.kind == DPB_OP_CONV && e->ops[pi].d.ip[9] == DPB_GATHER_NONE && !e->ops[pi].is_const) e->ops[pi].ln_next = (int)j;
      if (uses[d.out] == 1) {
        const int ci = user[d.out];
        const dpb_op_desc& cd = e->ops[ci].d;
        if (cd.kind == DPB_OP_CONV && cd.ip[9] == DPB_GATHER_NONE && cd.in0 == d.out && cd.w[1]) e->ops[ci].ln_prev = (int)j;
      }
    }
    for (size_t j = 0; j < e->ops.size(); ++j) {
      const dpb_op_desc& d = e->ops[j].d;
      // the primal GEGLU overwrites its input by the factors (G1, G2) (elementwise.hip): nothing else may read that buffer
      if (d.kind == DPB_OP_GEGLU && uses[d.in0] != 1) return bad("the input buffer of a GEGLU op must have no other consumer (the primal pass overwrites it in place)", (int)j);
      if (d.kind != DPB_OP_GEGLU || d.ip[1] != 64 || e->ops[j].is_const || getenv("DPB_NO_GEGLU_FUSE")) continue;   // (env: A/B tuning switch)
      const int pi = e->producer[d.in0];
      if (pi >= 0 && uses[d.in0] == 1) {
        const dpb_op_desc& pd = e->ops[pi].d;
        if (pd.kind == DPB_OP_CONV && pd.ip[9] == DPB_GATHER_NONE && pd.res < 0 && e->bufs[d.in0].kind == DPB_BUF_ACT) e->ops[pi].geglu_next = (int)j;
      }
      if (uses[d.out] == 1) {
        const int ci = user[d.out];
        const dpb_op_desc& cd = e->ops[ci].d;
        if (cd.kind == DPB_OP_CONV && cd.ip[9] == DPB_GATHER_NONE && cd.in0 == d.out) e->ops[ci].geglu_prev = (int)j;
      }
    }
    // Text-conditioned attention between a to_q and a to_out product that are its own (q read by nothing else, the output read by nothing else,
    // the three ops adjacent on the tape, whole [rows][C] buffers): the structural half of fold_route; the one-launch cross route is checked with the plan below
    for (size_t j = 1; j + 1 < e->ops.size(); ++j) {
      const dpb_op_desc& d = e->ops[j].d;
      if (d.kind != DPB_OP_ATTENTION || e->ops[j].is_const) continue;
      AttnPlan& p = e->plans[e->ops[j].attn];
      const int C = p.heads * p.d;
      if (!p.kv_const || p.causal || e->dtype == DT_F32 || p.oq != 0 || e->bufs[d.in0].C != C || e->bufs[d.out].C != C || p.Lk > 80) continue;
      const dpb_op_desc &qd = e->ops[j - 1].d, &od = e->ops[j + 1].d;
      auto plain = [&](const dpb_op_desc& c) {
        return c.kind == DPB_OP_CONV && c.ip[9] == DPB_GATHER_NONE && c.ip[6] == 1 && c.ip[2] == C && c.ip[5] == C && c.rowbias < 0 && c.w[1] &&
               e->bufs[c.in0].kind == DPB_BUF_ACT && e->bufs[c.out].kind == DPB_BUF_ACT;
      };
      if (!plain(qd) || qd.out != d.in0 || qd.res >= 0 || uses[d.in0] != 1 || e->ops[j - 1].is_const) continue;
      if (!plain(od) || od.in0 != d.out || uses[d.out] != 1) continue;
      p.q_op = (int)j - 1; p.o_op = (int)j + 1; p.fold_ok = true;
    }
    e->skip.assign(e->ops.size(), 0);
  }
  // ---------------- memory plan
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes); return o; };
  const size_t es = e->es;
  for (auto& b : e->bufs) {
    size_t n = e->maxB;                             // SHARED buffers too: one row per sample when the samples' timesteps differ (dpb_primal_t)
    b.p_off = take(n * b.rows * (size_t)b.C * es);
  }
  for (auto& b : e->bufs)
    if (!b.is_const) b.t_off = take((size_t)e->maxT * b.rows * b.C * es);
  for (auto& b : e->bufs)
    if (!b.is_const) b.g_off = b.g_off0 = take((size_t)e->maxT * b.rows * b.C * es);
  size_t s1 = 0, s2 = 0, t1 = 0, dv = 0, ctmp = 0, maxrc = 0;
  for (auto& op : e->ops) {
    const dpb_op_desc& d = op.d;
    if (d.kind == DPB_OP_ATTENTION) {
      AttnPlan& p = e->plans[op.attn];
      const size_t H = p.heads;
      // long bf16 self-attention layers run the flash-style kernels (attn_fused.hip): no L x L object is ever stored
      p.fused = !p.causal && fused_attention_supported(e->dtype, p.d, p.Lq, p.kv_const) && !getenv("DPB_NO_FUSED_ATTN") &&
                p.Lq >= (getenv("DPB_FUSED_ATTN_MIN_L") ? atoi(getenv("DPB_FUSED_ATTN_MIN_L")) : 64) &&       // tuning override (256: the 8x8 level back on the materialised path)
                e->bufs[d.in0].C == e->bufs[d.in1].C && e->bufs[d.in0].C == e->bufs[d.in2].C;
      p.cross = !p.causal && cross_attention_supported(e->dtype, p.d, p.Lq, p.Lk, p.kv_const) && !getenv("DPB_NO_CROSS_ATTN") &&
                e->bufs[d.in1].C == e->bufs[d.in2].C;
      if (!p.fused) p.P = take((size_t)e->maxB * H * p.Lq * p.Lkp * es);
      p.fold_ok = p.fold_ok && p.cross;
      if (p.fold_ok) {                             // the folded route's operands and probabilities, for the one sample it serves; its scratch is S1
        const size_t C = H * p.d;
        p.Gt = take(H * 128 * C * es); p.F = take(H * 128 * C * es);
        p.Gk = take(C * 80 * H * es); p.Fk = take(C * 80 * H * es);
        p.Pf = take((size_t)p.Lq * H * 80 * sizeof(float));
        s1 = std::max(s1, (size_t)e->maxT * H * p.Lq * 80 * es);
        e->ops[p.q_op].fold_plan = e->ops[p.o_op].fold_plan = op.attn;
        e->ops[p.q_op].fold_role = 1; e->ops[p.o_op].fold_role = 2;
      }
      p.VT = take((size_t)e->maxB * H * p.d * p.Lkp * es);
      p.KT = take((size_t)e->maxB * H * p.d * p.Lkp * es);
      if (!p.fused) s1 = std::max(s1, (size_t)e->maxT * H * p.Lq * p.Lkp * es);
      size_t lmax = std::max(p.Lqp, p.Lkp);
      t1 = std::max(t1, (size_t)e->maxT * H * p.d * lmax * es);
      if (p.fused) p.stats = take((size_t)e->maxB * H * p.Lq * 2 * sizeof(float));
      if (!p.kv_const) {
        if (!p.fused) p.PT = take((size_t)e->maxB * H * p.Lk * p.Lqp * es);
        p.QT = take((size_t)e->maxB * H * p.d * p.Lqp * es);
        if (!p.fused) s2 = std::max(s2, (size_t)e->maxT * H * p.Lk * p.Lqp * es);
        dv = std::max(dv, (size_t)e->maxT * H * p.Lq * sizeof(float));
      }
    } else if (d.kind == DPB_OP_GROUPNORM) {
      op.pstats = e->pstats_bytes;
      e->pstats_bytes += (size_t)e->maxB * d.ip[0] * 2 * sizeof(double);
      if (!op.is_const) {
        op.tstats = e->tstats_bytes;
        e->tstats_bytes += (size_t)e->maxT * d.ip[0] * 2 * sizeof(double);
      }
      if (gn_modulated(d)) op.aff = take((size_t)2 * e->maxB * e->bufs[d.in0].C * sizeof(float));
    } else if (d.kind == DPB_OP_CONV && d.ip[9] == DPB_GATHER_UPCONV && !op.is_const) {
      ctmp = std::max(ctmp, (size_t)e->maxT * d.ip[3] * d.ip[4] * e->bufs[d.in0].C * es);
    }
  }
  for (auto& b : e->bufs) maxrc = std::max(maxrc, (size_t)b.rows * b.C);
  e->pstats_off = take(e->pstats_bytes);
  e->tstats_off = take(e->tstats_bytes);
  {  // GroupNorm statistics scratch: one partial per (sample or tangent, block, group); a launch uses at most max(512, HW / 8) blocks in all
    size_t need = 0;
    for (auto& op : e->ops)
      if (op.d.kind == DPB_OP_GROUPNORM) {
        const size_t hw = e->bufs[op.d.in0].rows, nmax = (size_t)std::max(e->maxB, e->maxT);
        const size_t blocks = std::max<size_t>(nmax * ((hw + 7) / 8), 1);          // ppb >= 8
        need = std::max(need, std::min<size_t>(blocks, std::max<size_t>(1024, nmax * ((hw + 63) / 64))) * 2 * op.d.ip[0] * sizeof(float));
      }
    e->gnpart_bytes = need;
    e->gnpart = take(need);
    e->gnticket = take(sizeof(int) * (size_t)std::max(e->maxB, e->maxT));
  }
  for (auto& op : e->ops)
    if (op.d.kind == DPB_OP_GROUPNORM) { op.pstats += e->pstats_off; op.tstats += e->tstats_off; }
  e->S1 = take(s1); e->S2 = take(s2); e->T1 = take(t1); e->Dv = take(dv); e->convtmp = take(ctmp);
  const size_t nio = (size_t)std::max(e->maxB, e->maxT) * maxrc * sizeof(float);
  e->io_in = take(nio);
  e->io_out = take(nio);
  e->orth_stride = align_up(orth_scratch_bytes(std::min(ORTH_MAX_RANK, std::max(56, e->maxT)), (long)e->bufs[e->x_buf].rows * e->x_channels));   // k <= max_tangents
  e->orth = take(e->orth_stride * (size_t)e->maxB);
  e->slab = take(e->slab_bytes);
  e->zeros = take(256);
  const size_t nx = (size_t)e->bufs[e->x_buf].rows * e->x_channels;
  e->pbW = take((size_t)e->maxT * nx * sizeof(float));
  e->ws_bytes = off;
  e->ginit.assign(nb, 0);
  e->act_cache.assign(nb, std::vector<char>());
  if (!seed_flags(e, e->x_buf)) { delete e; return -1; }
  *out = e;
  return 0;
}

void dpb_engine_destroy(dpb_engine* e) {
  if (e && e->gexec) (void)hipGraphExecDestroy(e->gexec);
  delete e;
}

int dpb_engine_set_stream(dpb_engine* e, void* s) {
  if (!e) return fail("null engine");
  e->stream = (hipStream_t)s;
  return 0;
}

size_t dpb_engine_workspace_bytes(const dpb_engine* e) { return e ? e->ws_bytes : 0; }

int dpb_engine_set_workspace(dpb_engine* e, void* ws, size_t bytes) {
  if (!e || !ws) return fail("null argument");
  if (bytes < e->ws_bytes) return fail("workspace too small: %zu < %zu", bytes, e->ws_bytes);
  if ((uintptr_t)ws % 256) return fail("workspace must be 256-byte aligned");
  e->ws = (char*)ws;
  e->cur_batch = 0;
  DPB_CHECK(hipMemsetAsync(ws, 0, e->ws_bytes, e->stream));
  return 0;
}

// The shifted forwards, right after op producer[f.seed]: the tap becomes `groups` shifted copies of its xb rows, then (shared prefix, groups > 1) the
// first xb samples of every buffer the rest of the pass still reads are copied as one block to each of the other groups (a buffer is [batch]
// contiguous samples, so the block of xb samples is one "row" of the copy; xb == 1: sample 0 broadcast to the batch).  That set comes from the tape:
// the per-sample inputs (op_inputs) of the ops in (producer[f.seed], last] that were written at or before producer[f.seed] or are network inputs
// (ctx) -- the skips, the net-wide K/V projection of the context.  SHARED buffers (time-embedding path, row biases) have one copy for any batch; the
// tap itself is written by shift_tap.  Nothing else crosses the seam: a primal normalisation op computes its statistics from its own input, it takes
// none from that input's producer.
static int shift_seed(dpb_engine* e, const Forward& f, int last) {
  const int src = f.seed, ps = e->producer[src], xb = f.xbatch;
  const Buf& bs = e->bufs[src];
  if (int r = launch_shift_tap(e->dtype, e->P(src), f.u, f.dir, f.scale, xb, f.groups, bs.C, bs.Cv, bs.rows, e->stream)) return r;
  if (f.groups == 1) return 0;
  std::vector<char> seen(e->bufs.size(), 0);
  std::vector<void*> ptr;
  std::vector<size_t> bytes;
  for (int i = ps + 1; i <= last; ++i)
    for (int b : op_inputs(e->ops[i].d)) {
      if (b == src || seen[b] || e->bufs[b].kind == DPB_BUF_SHARED || e->producer[b] > ps) continue;
      seen[b] = 1;
      ptr.push_back(e->P(b));
      bytes.push_back((size_t)e->bufs[b].rows * e->bufs[b].C * e->es * xb);
    }
  return launch_replicate_rows(ptr.data(), bytes.data(), (int)ptr.size(), f.groups, e->stream);
}

// the sinusoidal timestep embedding, computed on the host in fp32 exactly as the reference frameworks do (diffusion.py:783-804 / diffusers
// Timesteps); emb: C(temb_buf) floats, the padding beyond temb_dim left as it is
static void temb_row(const dpb_engine* e, float t, float* emb) {
  const int half = e->temb_dim / 2;
  for (int i = 0; i < half; ++i) {
    float fr;
    if (e->temb_hm1) fr = expf((float)i * (float)(-(log(10000.0) / (double)(half - 1))));   // diffusion.py:797-798
    else fr = expf(((float)(-log(10000.0)) * (float)i) / (float)half);                      // diffusers get_timestep_embedding
    float ang = t * fr;
    float s = sinf(ang), c = cosf(ang);
    if (e->temb_flip) { emb[i] = c; emb[half + i] = s; } else { emb[i] = s; emb[half + i] = c; }
  }
}

// tv: null -- the batch shares t; else `batch` DISTINCT timesteps (dpb_primal_t has validated them and the tape): sample b's embedding goes to row b
// of P(temb_buf) and every SHARED op runs once per sample, at the M = 1 of the shared-timestep pass, into that sample's row
static int primal_pass(dpb_engine* e, const float* x, int batch, float t, const float* ctx, int upto_buf, const Forward& f, const float* tv = nullptr) {
  if (!e || !x) return fail("null argument");
  if (!e->ws) return fail("workspace not set (dpb_engine_set_workspace)");
  if (batch < 1 || batch > e->maxB) return fail("batch=%d outside [1,%d]", batch, e->maxB);
  if (upto_buf < 0 || upto_buf >= (int)e->bufs.size() || e->producer[upto_buf] < 0) return fail("invalid upto buffer %d", upto_buf);
  const LaunchSpan span(e);
  e->flops = 0; e->gbytes = 0;
  Pass ps(e, MODE_PRIMAL, upto_buf, e->x_buf, seed_flags(e, e->x_buf));
  ps.fwd = f;
  ps.per_sample_t = tv != nullptr;
  const Buf& bx = e->bufs[e->x_buf];
  const int xb = f.u ? f.xbatch : batch;           // samples of x / ctx (a shifted forward with a shared prefix: batch / groups)
  if (int r = launch_nchw_to_nhwc(e->dtype, x, e->P(e->x_buf), xb, e->x_channels, bx.rows, bx.C, e->stream)) return r;
  if (e->ctx_buf >= 0) {
    if (!ctx) return fail("this network needs ctx (encoder_hidden_states)");
    const Buf& bc = e->bufs[e->ctx_buf];
    // ctx is already [batch][rows][Cv] channel-last (Cv = un-padded width): cast (and zero-pad to C) via the nchw kernel with HW=1
    if (int r = launch_nchw_to_nhwc(e->dtype, ctx, e->P(e->ctx_buf), xb * bc.rows, bc.Cv, 1, bc.C, e->stream)) return r;
  }
  if (e->temb_buf >= 0 && !f.temb_resident) {
    // uploaded through the io staging area: one copy and one synchronisation, however many timesteps
    const int nrow = tv ? batch : 1;
    const size_t C = e->bufs[e->temb_buf].C;
    std::vector<float> emb(nrow * C, 0.f);
    for (int b = 0; b < nrow; ++b) temb_row(e, tv ? tv[b] : t, emb.data() + b * C);
    float* stage = (float*)(e->ws + e->io_in);
    DPB_CHECK(hipMemcpyAsync(stage, emb.data(), emb.size() * sizeof(float), hipMemcpyHostToDevice, e->stream));
    DPB_CHECK(hipStreamSynchronize(e->stream));   // emb is a host temporary
    for (int b = 0; b < nrow; ++b)                // (one launch per row: the launch of the shared-timestep pass, whatever the batch)
      if (int r = launch_nchw_to_nhwc(e->dtype, stage + b * C, e->P(e->temb_buf) + b * C * e->es, 1, (int)C, 1, (int)C, e->stream)) return r;
  }
  if (e->pstats_bytes && !gn_deterministic()) DPB_CHECK(hipMemsetAsync(e->ws + e->pstats_off, 0, e->pstats_bytes, e->stream));   // atomic statistics path accumulates
  e->cur_batch = batch;
  e->pend.on = false;
  const int last = e->producer[upto_buf];
  const int seed_op = f.seed >= 0 ? e->producer[f.seed] : -1;
  e->primal_last = -1;
  for (auto& p : e->plans) p.fold_live = false;    // the folded operands belong to the primal pass that built them
  std::fill(e->skip.begin(), e->skip.end(), 0);
  for (int i = 0; i <= last; ++i) {
    if (e->skip[i]) continue;                      // (forward only: a GEGLU applied by the epilogue of the FF-in product)
    const int reps = tv && e->bufs[e->ops[i].d.out].kind == DPB_BUF_SHARED ? batch : 1;   // a SHARED op under per-sample timesteps: once per sample
    for (ps.srow = 0; ps.srow < reps; ++ps.srow)
      if (int r = run_op(e, e->ops[i], ps, i <= seed_op ? xb : batch)) return r;
    ps.srow = 0;
    if (int r = fill_affine(e, i, ps, batch)) return r;
    if (i == seed_op && f.u) {                     // a shifted forward: the tap just computed becomes the shifted copies of its xb rows
      if (int r = shift_seed(e, f, last)) return r;
    } else if (i == seed_op) {                     // dpb_forward_from: the caller's activation replaces the one just computed
      const Buf& bs = e->bufs[f.seed];
      if (int r = launch_nchw_to_nhwc(e->dtype, f.h, e->P(f.seed), batch, bs.Cv, bs.rows, bs.C, e->stream)) return r;
    }
  }
  if (f.stash) e->primal_last = last;
  return 0;
}

int dpb_primal(dpb_engine* e, const float* x, int batch, float t, const float* ctx, int upto_buf) {
  return primal_pass(e, x, batch, t, ctx, upto_buf, Forward());
}

// The checks of the per-sample entry points.  *tv: null when every entry of t equals t[0] (the call IS the shared-timestep one), else t.
static int check_timesteps(dpb_engine* e, int batch, const float* t, const float** tv) {
  if (!e || !t) return fail("null argument");
  if (batch < 1 || batch > e->maxB) return fail("batch=%d outside [1,%d]", batch, e->maxB);
  *tv = nullptr;
  for (int b = 0; b < batch; ++b) {
    if (!isfinite(t[b])) return fail("t[%d] is not finite", b);
    if (t[b] != t[0]) *tv = t;
  }
  if (!*tv) return 0;
  if (e->temb_buf < 0 || !e->temb_read) return fail("distinct timesteps on a network without a timestep embedding (no op reads temb_buf): its samples cannot differ in t");
  if (e->bufs[e->temb_buf].kind != DPB_BUF_SHARED || e->bufs[e->temb_buf].rows != 1) return fail("distinct timesteps need temb_buf to be a SHARED buffer of one row");
  if (!e->per_sample_t_why.empty()) return fail("distinct timesteps are unsupported on this tape: %s", e->per_sample_t_why.c_str());
  return 0;
}

int dpb_primal_t(dpb_engine* e, const float* x, int batch, const float* t, const float* ctx, int upto_buf) {
  const float* tv;
  if (int r = check_timesteps(e, batch, t, &tv)) return r;
  return primal_pass(e, x, batch, t[0], ctx, upto_buf, Forward(), tv);
}

// dpb_forward and the entry points built on it: a primal pass that keeps no stash (f.stash == false), read out at upto_buf
static int forward_pass(dpb_engine* e, const float* x, int batch, float t, const float* ctx, int upto_buf, int channels, float* out, const Forward& f,
                        const float* tv = nullptr) {
  if (!e || !out) return fail("null argument");
  int r = primal_pass(e, x, batch, t, ctx, upto_buf, f, tv);
  if (!r) r = dpb_read_buffer(e, upto_buf, channels, out);
  e->cur_batch = 0;                                // no stash was kept: dpb_jvp / dpb_vjp / dpb_pullback_iterate refuse until the next dpb_primal
  return r;
}

int dpb_forward(dpb_engine* e, const float* x, int batch, float t, const float* ctx, int upto_buf, int channels, float* out) {
  Forward f;
  f.stash = false;
  return forward_pass(e, x, batch, t, ctx, upto_buf, channels, out, f);
}

int dpb_forward_t(dpb_engine* e, const float* x, int batch, const float* t, const float* ctx, int upto_buf, int channels, float* out) {
  const float* tv;
  if (int r = check_timesteps(e, batch, t, &tv)) return r;
  Forward f;
  f.stash = false;
  return forward_pass(e, x, batch, t[0], ctx, upto_buf, channels, out, f, tv);
}

int dpb_forward_from(dpb_engine* e, const float* x, int batch, float t, const float* ctx, int src_buf, const float* h, int dst_buf, int channels,
                     float* out) {
  if (!e || !out || !h) return fail("null argument");
  if (int r = check_pair(e, src_buf, dst_buf, FOR_FORWARD)) return r;
  Forward f;
  f.stash = false; f.seed = src_buf; f.h = h;
  return forward_pass(e, x, batch, t, ctx, dst_buf, channels, out, f);
}

int dpb_forward_shift(dpb_engine* e, const float* x, int xbatch, int batch, float t, const float* ctx, int src_buf, const float* u, int nu,
                      const int32_t* dir, const float* scale, int dst_buf, int channels, float* out) {
  if (!e || !x || !out || !dir || !scale) return fail("null argument");
  e->cur_batch = 0;                                // as dpb_forward: whatever happens below, the primal state is gone
  if (batch < 1 || batch > e->maxB) return fail("batch=%d outside [1,%d]", batch, e->maxB);
  if (xbatch != 1 && xbatch != batch) return fail("xbatch=%d must be 1 (one sample shared by the batch) or batch=%d", xbatch, batch);
  if (nu < 1) return fail("nu=%d: at least one direction is needed", nu);
  if (!u) return fail("null argument");
  for (int b = 0; b < batch; ++b)
    if (dir[b] < -1 || dir[b] >= nu) return fail("dir[%d]=%d outside [-1,%d) (-1: no shift)", b, dir[b], nu);
  if (int r = check_pair(e, src_buf, dst_buf, FOR_FORWARD)) return r;
  Forward f;
  f.stash = false; f.seed = src_buf; f.u = u; f.dir = dir; f.scale = scale; f.xbatch = xbatch; f.groups = batch / xbatch;
  return forward_pass(e, x, batch, t, ctx, dst_buf, channels, out, f);
}

// The rows of a call that follows h-space directions: dir[r] in [lo, nu) (lo = -1: a row may go unshifted) and every per-row scalar finite
struct RowScalars { const char* name; const float* v; };
static int check_dirs(const char* who, int n, int nu, int lo, const int32_t* dir, std::initializer_list<RowScalars> scalars) {
  if (nu < 1) return fail("%s: nu=%d: at least one direction is needed", who, nu);
  for (int r = 0; r < n; ++r) {
    if (dir[r] < lo || dir[r] >= nu) return fail("%s: dir[%d]=%d outside [%d,%d)%s", who, r, dir[r], lo, nu, lo < 0 ? " (-1: no shift)" : "");
    for (const RowScalars& s : scalars)
      if (!isfinite(s.v[r])) return fail("%s: %s[%d] is not finite", who, s.name, r);
  }
  return 0;
}

// the checks of dpb_forward_shift_groups: the shape of the grouped batch and its rows
static int check_groups(dpb_engine* e, const char* who, int xbatch, int groups, int nu, const int32_t* dir, const float* scale) {
  if (xbatch < 1) return fail("%s: xbatch=%d < 1", who, xbatch);
  if (groups < 1) return fail("%s: groups=%d < 1", who, groups);
  if (groups > SHIFT_MAX_ROWS) return fail("%s: groups=%d above %d", who, groups, SHIFT_MAX_ROWS);
  if ((long)xbatch * groups > e->maxB) return fail("%s: xbatch * groups = %d * %d rows above max_batch=%d", who, xbatch, groups, e->maxB);
  return check_dirs(who, xbatch * groups, nu, -1, dir, {{"scale", scale}});
}

// ---- the frame of the entry points that run several passes over a caller's scratch (dpb_local_pca_sample, dpb_inv_jac_chain, dpb_hguide_chain)
// the scratch, carved into 256-byte aligned pieces: take() is the offset of the next one, off the total
struct ScratchLayout {
  size_t off = 0;
  size_t take(size_t bytes) { const size_t o = off; off += align_up(bytes); return o; }
};

static int check_scratch(const char* who, const char* sizer, const void* scratch, size_t bytes, size_t need) {
  if ((uintptr_t)scratch % 256) return fail("%s: scratch must be 256-byte aligned", who);
  if (bytes < need) return fail("%s: scratch of %zu bytes, %s = %zu", who, bytes, sizer, need);
  return 0;
}

// a tap a chain can follow: an activation produced by an op that depends on x
static int check_chain_tap(const dpb_engine* e, const char* who, int tap) {
  if (tap < 0 || tap >= (int)e->bufs.size() || e->producer[tap] < 0 || e->bufs[tap].kind != DPB_BUF_ACT)
    return fail("%s: invalid tap buffer %d (an activation produced by an op)", who, tap);
  if (e->bufs[tap].is_const) return fail("%s: tap buffer %d does not depend on x", who, tap);
  return 0;
}

// The statistics of a call made of several passes: opened before the first (the sub-passes' LaunchSpans overwrite n_launch as they go), add() after each
// pass that counts flops and bytes, close() when the call ends: its totals, and no primal state is left behind.
struct CallTotals {
  dpb_engine* e;
  const long at = launch_count;
  double fl = 0, gb = 0;
  explicit CallTotals(dpb_engine* e_) : e(e_) {}
  void add() { fl += e->flops; gb += e->gbytes; }
  int close(int r) {
    e->cur_batch = 0;
    e->primal_last = -1;
    e->n_launch = launch_count - at; e->flops = fl; e->gbytes = gb;
    return r;
  }
};

int dpb_forward_shift_groups(dpb_engine* e, const float* x, int xbatch, int groups, float t, const float* ctx, int src_buf, const float* u, int nu,
                             const int32_t* dir, const float* scale, int dst_buf, int channels, float* out) {
  if (!e || !x || !out || !dir || !scale || !u) return fail("dpb_forward_shift_groups: null argument");
  e->cur_batch = 0;                                // as dpb_forward: whatever happens below, the primal state is gone
  if (int r = check_groups(e, "dpb_forward_shift_groups", xbatch, groups, nu, dir, scale)) return r;
  if (int r = check_pair(e, src_buf, dst_buf, FOR_FORWARD)) return r;
  Forward f;
  f.stash = false; f.seed = src_buf; f.u = u; f.dir = dir; f.scale = scale; f.xbatch = xbatch; f.groups = groups;
  return forward_pass(e, x, xbatch * groups, t, ctx, dst_buf, channels, out, f);
}

int dpb_read_buffer(dpb_engine* e, int buf, int channels, float* out) {
  if (!e || !out) return fail("null argument");
  if (buf < 0 || buf >= (int)e->bufs.size()) return fail("bad buffer %d", buf);
  const Buf& b = e->bufs[buf];
  if (channels < 1 || channels > b.C) return fail("bad channel count");
  int n = b.kind == DPB_BUF_SHARED ? 1 : e->cur_batch;
  if (n < 1) return fail("no primal state to read (dpb_forward invalidates it; run dpb_primal first)");
  return launch_nhwc_to_nchw(e->dtype, e->P(buf), out, n, channels, b.rows, b.C, e->stream);
}

// U == nullptr (dpb_pullback_iterate, every iteration but the last): the tangent of the tap stays in T(tap); the adjoint pass takes it from there
// src: the seed buffer (x_buf: the encoder Jacobian); ops up to producer[src] and ops whose output does not depend on src do not run
static int jvp_pass(dpb_engine* e, int src, int tap, const float* V, int nt, float* U) {
  if (!e || !V) return fail("null argument");
  const char* flags;
  if (int r = check_pass(e, src, tap, nt, &flags)) return r;
  const Pass ps(e, MODE_TANGENT, tap, src, flags);
  const LaunchSpan span(e);
  e->flops = 0; e->gbytes = 0;
  const Buf& bx = e->bufs[src];
  if (int r = launch_nchw_to_nhwc(e->dtype, V, e->T(src), nt, seed_channels(e, src), bx.rows, bx.C, e->stream)) return r;
  if (e->tstats_bytes && !gn_deterministic()) DPB_CHECK(hipMemsetAsync(e->ws + e->tstats_off, 0, e->tstats_bytes, e->stream));   // atomic statistics accumulate
  const int last = e->producer[tap];
  std::fill(e->skip.begin(), e->skip.end(), 0);
  e->pend.on = false;
  for (int i = e->producer[src] + 1; i <= last; ++i) {
    if (!ps.oact[i] || e->skip[i]) continue;
    if (int r = run_op(e, e->ops[i], ps, nt)) return r;
  }
  if (int r = flush_pending(e)) return r;
  if (!U) return 0;
  const Buf& bt = e->bufs[tap];
  return launch_nhwc_to_nchw(e->dtype, e->T(tap), U, nt, bt.Cv, bt.rows, bt.C, e->stream);
}

int dpb_jvp(dpb_engine* e, int tap, const float* V, int nt, float* U) {
  if (!U) return fail("null argument");
  return jvp_pass(e, e ? e->x_buf : -1, tap, V, nt, U);
}

int dpb_jvp_between(dpb_engine* e, int src_buf, int dst_buf, const float* V, int nt, float* U) {
  if (!e || !U) return fail("null argument");
  return jvp_pass(e, src_buf, dst_buf, V, nt, U);
}

// U == nullptr: the cotangent seed IS the tangent the last jvp_pass left in T(tap) -- its storage is handed to G(tap) for this pass (the fp32 NCHW round
// trip through U is the identity on 16-bit and fp32 values alike, so the results are bitwise those of the two conversion kernels it replaces)
static int vjp_pass(dpb_engine* e, int src, int tap, const float* U, int nt, float* W) {
  if (!e || !W) return fail("null argument");
  const char* flags;
  if (int r = check_pass(e, src, tap, nt, &flags)) return r;
  const Pass ps(e, MODE_ADJOINT, tap, src, flags);
  const LaunchSpan span(e);
  e->flops = 0; e->gbytes = 0;
  const Buf& bt = e->bufs[tap];
  std::fill(e->ginit.begin(), e->ginit.end(), 0);
  for (auto& b : e->bufs) b.g_off = b.g_off0;
  if (U) {
    if (int r = launch_nchw_to_nhwc(e->dtype, U, e->G(tap), nt, bt.Cv, bt.rows, bt.C, e->stream)) return r;
  } else {
    e->bufs[tap].g_off = e->bufs[tap].t_off;       // restored from g_off0 at the start of the next adjoint pass
  }
  e->ginit[tap] = 1;
  if (e->tstats_bytes && !gn_deterministic()) DPB_CHECK(hipMemsetAsync(e->ws + e->tstats_off, 0, e->tstats_bytes, e->stream));
  e->pend.on = false;
  for (int i = e->producer[tap]; i > e->producer[src]; --i) {   // (the seed's producer and everything before it: upstream of the pass)
    const Op& op = e->ops[i];
    if (!ps.oact[i] || !e->ginit[op.d.out]) continue;
    if (int r = run_op(e, op, ps, nt)) return r;
  }
  if (int r = flush_pending(e)) return r;
  if (!e->ginit[src]) {
    for (auto& b : e->bufs) b.g_off = b.g_off0;
    return src == e->x_buf ? fail("tap buffer %d is not connected to x", tap) : fail("dst buffer %d is not connected to source buffer %d", tap, src);
  }
  const Buf& bx = e->bufs[src];
  const int r = launch_nhwc_to_nchw(e->dtype, e->G(src), W, nt, seed_channels(e, src), bx.rows, bx.C, e->stream);
  // Invariant of Buf::g_off / t_off: between passes every buffer's cotangent storage is its own (g_off == g_off0).  Inside the pass the residual adjoint
  // swaps g_off between buffers and U == nullptr lends the tap's TANGENT storage to its cotangent; undo both here so that nothing that reads G() or
  // T(tap) after the pass (a debug read, a later feature) sees aliased data.  (The launch above is already enqueued with the pointer it needs.)
  for (auto& b : e->bufs) b.g_off = b.g_off0;
  return r;
}

int dpb_vjp(dpb_engine* e, int tap, const float* U, int nt, float* W) {
  if (!U) return fail("null argument");
  return vjp_pass(e, e ? e->x_buf : -1, tap, U, nt, W);
}

int dpb_vjp_between(dpb_engine* e, int src_buf, int dst_buf, const float* U, int nt, float* W) {
  if (!e || !U) return fail("null argument");
  return vjp_pass(e, src_buf, dst_buf, U, nt, W);
}

static OrthArgs orth_args(const float* W, const float* Vprev, float* V, float* s, float* conv, void* scratch, size_t scratch_bytes, int k, long N) {
  OrthArgs a;
  a.W = W; a.Vprev = Vprev; a.V = V; a.s = s; a.conv = conv; a.scratch = (double*)scratch; a.scratch_bytes = scratch_bytes; a.k = k; a.N = N;
  return a;
}

int dpb_orth(const float* W, const float* Vprev, float* V, float* s, float* conv, void* scratch, int k, int64_t N, void* stream) {
  if (!W || !Vprev || !V || !s || !conv || !scratch) return fail("null argument");
  return launch_orth(orth_args(W, Vprev, V, s, conv, scratch, orth_scratch_bytes(k, N) /* the caller's contract (include/dpb.h) */, k, N), (hipStream_t)stream);
}

int dpb_orth_checked(const float* W, const float* Vprev, float* V, float* s, float* conv, void* scratch, size_t scratch_bytes, int k, int64_t N,
                     void* stream) {
  if (!W || !Vprev || !V || !s || !conv || !scratch) return fail("null argument");
  if (k < 1 || k > ORTH_MAX_RANK || N < 1) return fail("dpb_orth: k=%d outside [1,%d] or N=%lld < 1", k, ORTH_MAX_RANK, (long long)N);
  const size_t need = orth_scratch_bytes(k, N);
  if (scratch_bytes < need) return fail("dpb_orth: scratch of %zu bytes, dpb_orth_scratch_bytes(%d, %lld) = %zu", scratch_bytes, k, (long long)N, need);
  return launch_orth(orth_args(W, Vprev, V, s, conv, scratch, scratch_bytes, k, N), (hipStream_t)stream);
}

size_t dpb_orth_scratch_bytes(int k, int64_t N) { return (k < 1 || k > ORTH_MAX_RANK || N < 1) ? 0 : orth_scratch_bytes(k, N); }

// torch.pca_lowrank(H, q, center=True, niter) for the reference's global_pca_zt (src/utils/utils.py:978-1027; torch._lowrank._svd_lowrank +
// get_approximate_basis): pca.hip
size_t dpb_pca_scratch_bytes(int q, int64_t N, int64_t D) { return pca_scratch_bytes(q, N, D); }

int dpb_pca_lowrank(const float* H, int64_t N, int64_t D, const float* R, int q, int niter, float* u, float* s, void* scratch,
                    size_t scratch_bytes, void* stream) {
  if (!H || !R || !u || !s || (!scratch && scratch_bytes)) return fail("dpb_pca_lowrank: null argument");   // (no scratch: the size check below fails)
  return launch_pca_lowrank(H, N, D, R, q, niter, u, s, scratch, scratch_bytes, (hipStream_t)stream);
}

// Principal angles / geodesic distances between the saved local tangent spaces (the analysis run_sample_encoder_local_tangent_space_zt saves its
// bases for; the reference carries no code for it): angles.hip
int dpb_cross_gram(const float* X, const float* Y, double* G, int Ra, int Rb, int64_t N, void* stream) {
  if (!X || !G) return fail("dpb_cross_gram: null argument");
  return launch_cross_gram(X, Y, G, Ra, Rb, N, (hipStream_t)stream);
}

size_t dpb_subspace_angles_scratch_bytes(int Ba, int Bb, int k, int64_t N) { return subspace_angles_scratch_bytes(Ba, Bb, k, N); }

int dpb_subspace_angles(const float* A, const float* B, int Ba, int Bb, int k, int64_t N, float* theta, float* dist, void* scratch, size_t scratch_bytes,
                        void* stream) {
  if (!A || !theta || !dist || !scratch) return fail("dpb_subspace_angles: null argument");
  return launch_subspace_angles(A, B, Ba, Bb, k, N, theta, dist, scratch, scratch_bytes, (hipStream_t)stream);
}

// Parallel transport of principal directions from one tangent space to others (run_edit_parallel_transport, src/modules/edit.py:892-909): transport.hip
size_t dpb_transport_scratch_bytes(int D, int P, int k, int64_t N_h, int64_t N_x) { return transport_scratch_bytes(D, P, k, N_h, N_x); }

int dpb_transport_directions(const float* u_src, const float* u_dst, const float* vT_dst, const int32_t* pcs, int P, int D, int k, int64_t N_h,
                             int64_t N_x, float* vk, float* coef, float* coef_norm, void* scratch, size_t scratch_bytes, void* stream) {
  if (!u_src || !u_dst || !vT_dst || !pcs || !vk || !coef || !coef_norm || !scratch) return fail("dpb_transport_directions: null argument");
  return launch_transport_directions(u_src, u_dst, vT_dst, pcs, P, D, k, N_h, N_x, vk, coef, coef_norm, scratch, scratch_bytes, (hipStream_t)stream);
}

// Frechet (Karcher) mean on the Grassmannian of many local bases, the global basis of run_edit_global_frechet_mean_zt (src/modules/edit.py:951-1246):
// frechet.hip
size_t dpb_frechet_scratch_bytes(int B, int k, int64_t N, int max_iter) { return frechet_scratch_bytes(B, k, N, max_iter); }

int dpb_frechet_init(const float* X, int B, int k, int64_t N, int init, int max_iter, void* scratch, size_t scratch_bytes, void* stream) {
  if (!X || !scratch) return fail("dpb_frechet_init: null argument");
  return launch_frechet_init(X, B, k, N, max_iter, init, scratch, scratch_bytes, (hipStream_t)stream);
}

int dpb_frechet_iterate(int n_iter, double step, double tol, int B, int k, int64_t N, int max_iter, void* scratch, size_t scratch_bytes, void* stream) {
  if (!scratch) return fail("dpb_frechet_iterate: null argument");
  return launch_frechet_iterate(B, k, N, max_iter, n_iter, step, tol, scratch, scratch_bytes, (hipStream_t)stream);
}

int dpb_frechet_finish(const float* X, float* Y, float* weight, float* theta, double* info, int B, int k, int64_t N, int max_iter, void* scratch,
                       size_t scratch_bytes, void* stream) {
  if (!X || !Y || !weight || !theta || !info || !scratch) return fail("dpb_frechet_finish: null argument");
  return launch_frechet_finish(X, B, k, N, max_iter, Y, weight, theta, info, scratch, scratch_bytes, (hipStream_t)stream);
}

const double* dpb_frechet_ghat(int B, int k, int64_t N, int max_iter, const void* scratch) {
  if (!scratch) { fail("dpb_frechet_ghat: null argument"); return nullptr; }
  const double* g = frechet_ghat(B, k, N, max_iter, scratch);
  if (!g) fail("dpb_frechet_ghat: B=%d, k=%d, N=%lld, max_iter=%d is no Frechet problem", B, k, (long long)N, max_iter);
  return g;
}

int dpb_frechet_start(const double* Ct, int B, int k, int64_t N, int max_iter, void* scratch, size_t scratch_bytes, void* stream) {
  if (!Ct || !scratch) return fail("dpb_frechet_start: null argument");
  return launch_frechet_start(Ct, B, k, N, max_iter, scratch, scratch_bytes, (hipStream_t)stream);
}

// principal geodesic analysis of many local bases around a base point (geometry.grassmann_pga): pga.hip, on a Frechet scratch block after dpb_frechet_finish
size_t dpb_pga_scratch_bytes(int B, int members, int k, int64_t N, int J) { return pga_scratch_bytes(B, members, k, N, J); }

int dpb_pga_tangent_gram(int B, int members, int k, int64_t N, int max_iter, int J, void* frechet_scratch, size_t frechet_bytes, double* T, float* theta,
                         int32_t* state, void* scratch, size_t scratch_bytes, void* stream) {
  if (!frechet_scratch || !T || !theta || !state || !scratch) return fail("dpb_pga_tangent_gram: null argument");
  return launch_pga_tangent_gram(B, members, k, N, max_iter, J, frechet_scratch, frechet_bytes, T, theta, state, scratch, scratch_bytes, (hipStream_t)stream);
}

int dpb_pga_eig(const double* T, int B, int members, int k, int64_t N, int J, int M, int center, double* Wt, double* out, void* scratch, size_t scratch_bytes,
                void* stream) {
  if (!T || !Wt || !out || !scratch) return fail("dpb_pga_eig: null argument");
  return launch_pga_eig(T, B, members, k, N, J, M, center, Wt, out, scratch, scratch_bytes, (hipStream_t)stream);
}

int dpb_pga_combine(const float* X, const double* Wt, int rows, float* out, int B, int members, int k, int64_t N, int max_iter, int J, void* frechet_scratch,
                    size_t frechet_bytes, void* scratch, size_t scratch_bytes, void* stream) {
  if (!X || !Wt || !out || !frechet_scratch || !scratch) return fail("dpb_pga_combine: null argument");
  return launch_pga_combine(X, Wt, B, members, k, N, max_iter, J, rows, frechet_scratch, frechet_bytes, out, scratch, scratch_bytes, (hipStream_t)stream);
}

// the flag (extrinsic) mean of many local bases, the global basis of run_edit_global_flag_mean_zt: flagmean.hip
size_t dpb_flag_mean_scratch_bytes(int B, int k, int64_t N, int r, int max_iter) { return flag_mean_scratch_bytes(B, k, N, r, max_iter, true); }
size_t dpb_flag_mean_solver_bytes(int B, int k, int r, int max_iter) { return flag_mean_scratch_bytes(B, k, 0, r, max_iter, false); }

int dpb_flag_mean_init(const float* X, const double* Ghat, int B, int k, int64_t N, int r, uint64_t seed, int max_iter, void* scratch,
                       size_t scratch_bytes, void* stream) {
  if (!scratch || (X == nullptr) == (Ghat == nullptr)) return fail("dpb_flag_mean_init: null scratch, or not exactly one of X and Ghat given");
  return launch_flag_mean_init(X, Ghat, B, k, N, r, seed, max_iter, scratch, scratch_bytes, (hipStream_t)stream);
}

int dpb_flag_mean_iterate(int n_iter, double tol, const double* Ghat, int B, int k, int64_t N, int r, int max_iter, void* scratch, size_t scratch_bytes,
                          void* stream) {
  if (!scratch) return fail("dpb_flag_mean_iterate: null argument");
  return launch_flag_mean_iterate(Ghat, B, k, N, r, max_iter, n_iter, tol, scratch, scratch_bytes, (hipStream_t)stream);
}

int dpb_flag_mean_finish(const float* X, const double* Ghat, float* Y, float* weight, float* theta, double* Ct, double* info, int B, int k, int64_t N,
                         int r, int max_iter, void* scratch, size_t scratch_bytes, void* stream) {
  if (!weight || !theta || !Ct || !info || !scratch) return fail("dpb_flag_mean_finish: null argument");
  if ((X == nullptr) != (Y == nullptr) || (X == nullptr) == (Ghat == nullptr))
    return fail("dpb_flag_mean_finish: X and Y go together, and exactly one of X and Ghat is given");
  return launch_flag_mean_finish(X, Ghat, B, k, N, r, max_iter, Y, weight, theta, Ct, info, scratch, scratch_bytes, (hipStream_t)stream);
}

// the weighted flag mean and the flag median (geometry.flag_mean(weights=) / flag_median): flagmean.hip
size_t dpb_flag_median_scratch_bytes(int B, int k, int64_t N, int r, int max_iter) { return flag_median_scratch_bytes(B, k, N, r, max_iter, true); }
size_t dpb_flag_median_solver_bytes(int B, int k, int r, int max_iter) { return flag_median_scratch_bytes(B, k, 0, r, max_iter, false); }

int dpb_flag_median_init(const float* X, const double* Ghat, const double* member_weight, int B, int k, int64_t N, int r, uint64_t seed, int max_iter,
                         void* scratch, size_t scratch_bytes, void* stream) {
  if (!scratch || (X == nullptr) == (Ghat == nullptr)) return fail("dpb_flag_median_init: null scratch, or not exactly one of X and Ghat given");
  return launch_flag_median_init(X, Ghat, member_weight, B, k, N, r, seed, max_iter, scratch, scratch_bytes, (hipStream_t)stream);
}

int dpb_flag_median_iterate(int n_iter, double tol, const double* Ghat, int B, int k, int64_t N, int r, int max_iter, void* scratch, size_t scratch_bytes,
                            void* stream) {
  if (!scratch) return fail("dpb_flag_median_iterate: null argument");
  return launch_flag_median_iterate(Ghat, B, k, N, r, max_iter, n_iter, tol, scratch, scratch_bytes, (hipStream_t)stream);
}

int dpb_flag_median_round(double eps, double tol, int update, const double* Ghat, int B, int k, int64_t N, int r, int max_iter, void* scratch,
                          size_t scratch_bytes, void* stream) {
  if (!scratch) return fail("dpb_flag_median_round: null argument");
  return launch_flag_median_round(Ghat, B, k, N, r, max_iter, eps, tol, update, scratch, scratch_bytes, (hipStream_t)stream);
}

int dpb_flag_median_finish(const float* X, const double* Ghat, float* Y, float* weight, float* theta, double* Ct, double* member, double* info, int B, int k,
                           int64_t N, int r, int max_iter, void* scratch, size_t scratch_bytes, void* stream) {
  if (!weight || !theta || !Ct || !member || !info || !scratch) return fail("dpb_flag_median_finish: null argument");
  if ((X == nullptr) != (Y == nullptr) || (X == nullptr) == (Ghat == nullptr))
    return fail("dpb_flag_median_finish: X and Y go together, and exactly one of X and Ghat is given");
  return launch_flag_median_finish(X, Ghat, B, k, N, r, max_iter, Y, weight, theta, Ct, member, info, scratch, scratch_bytes, (hipStream_t)stream);
}

// the chordal affinity of two stacks of subspaces, and flag k-means on it (geometry.flag_affinity / flag_kmeans): flagkmeans.hip
size_t dpb_flag_affinity_scratch_bytes(int B, int k, int C, int r, int64_t N) { return flag_affinity_scratch_bytes(B, k, C, r, N); }

int dpb_flag_affinity(const float* A, const float* Y, int B, int k, int C, int r, int64_t N, double* aff, void* scratch, size_t scratch_bytes, void* stream) {
  if (!A || !Y || !aff || !scratch) return fail("dpb_flag_affinity: null argument");
  return launch_flag_affinity(A, Y, B, k, C, r, N, aff, scratch, scratch_bytes, (hipStream_t)stream);
}

size_t dpb_flag_kmeans_scratch_bytes(int B, int k, int64_t N, int C, int r) { return flag_kmeans_scratch_bytes(B, k, N, C, r); }
size_t dpb_flag_kmeans_host_bytes(int B, int k, int64_t N, int C, int r) { return flag_kmeans_host_bytes(B, k, N, C, r); }

const double* dpb_flag_kmeans_affinity(int B, int k, int64_t N, int C, int r, const void* scratch) {
  const double* a = scratch ? flag_kmeans_affinity(B, k, N, C, r, scratch) : nullptr;
  if (!a) set_error("dpb_flag_kmeans_affinity: null scratch, or B=%d, k=%d, N=%ld, C=%d, r=%d is no flag k-means problem", B, k, (long)N, C, r);
  return a;
}

int dpb_flag_kmeans_init(const float* X, int B, int k, int64_t N, int C, int r, const int32_t* seeds, int n_seeds, void* scratch, size_t scratch_bytes,
                         void* stream) {
  if (!X || !seeds || !scratch) return fail("dpb_flag_kmeans_init: null argument");
  return launch_flag_kmeans_init(X, B, k, N, C, r, seeds, n_seeds, scratch, scratch_bytes, (hipStream_t)stream);
}

int dpb_flag_kmeans_gather(int c, int n_c, double* Gc, int B, int k, int64_t N, int C, int r, void* scratch, size_t scratch_bytes, void* stream) {
  if (!Gc || !scratch) return fail("dpb_flag_kmeans_gather: null argument");
  return launch_flag_kmeans_gather(B, k, N, C, r, c, n_c, Gc, scratch, scratch_bytes, (hipStream_t)stream);
}

int dpb_flag_kmeans_set_centre(int c, int n_c, const double* Ct, int B, int k, int64_t N, int C, int r, void* scratch, size_t scratch_bytes, void* stream) {
  if (!Ct || !scratch) return fail("dpb_flag_kmeans_set_centre: null argument");
  return launch_flag_kmeans_set_centre(B, k, N, C, r, c, n_c, Ct, scratch, scratch_bytes, (hipStream_t)stream);
}

int dpb_flag_kmeans_assign(int apply, int B, int k, int64_t N, int C, int r, void* scratch, size_t scratch_bytes, void* stream) {
  if (!scratch) return fail("dpb_flag_kmeans_assign: null argument");
  return launch_flag_kmeans_assign(B, k, N, C, r, apply, scratch, scratch_bytes, (hipStream_t)stream);
}

int dpb_flag_kmeans_finish(const float* X, float* Y, int B, int k, int64_t N, int C, int r, void* scratch, size_t scratch_bytes, void* stream) {
  if (!X || !Y || !scratch) return fail("dpb_flag_kmeans_finish: null argument");
  return launch_flag_kmeans_finish(X, B, k, N, C, r, Y, scratch, scratch_bytes, (hipStream_t)stream);
}

// The Hungarian-matched mean of local bases, the global basis of run_edit_global_hungarian_mean_zt (src/modules/edit.py:1249-1514): hungarian.hip
size_t dpb_linear_assignment_scratch_bytes(int B, int k) { return linear_assignment_scratch_bytes(B, k); }

int dpb_linear_assignment(const double* cost, int B, int k, int32_t* col_of_row, double* total, void* scratch, size_t scratch_bytes, void* stream) {
  if (!cost || !col_of_row || !total || !scratch) return fail("dpb_linear_assignment: null argument");
  return launch_linear_assignment(cost, B, k, col_of_row, total, scratch, scratch_bytes, (hipStream_t)stream);
}

size_t dpb_matched_mean_scratch_bytes(int B, int k, int64_t N) { return matched_mean_scratch_bytes(B, k, N); }

int dpb_matched_mean(const float* X, int B, int k, int64_t N, const float* anchor, int init, int distance, float* Y, int32_t* perm, int32_t* sign,
                     double* info, void* scratch, size_t scratch_bytes, void* stream) {
  if (!X || !Y || !perm || !sign || !info || !scratch) return fail("dpb_matched_mean: null argument");
  return launch_matched_mean(X, B, k, N, anchor, init, distance, Y, perm, sign, info, scratch, scratch_bytes, (hipStream_t)stream);
}

int dpb_row_sumsq(const float* X, int64_t rows, int64_t N, double* ss, void* stream) {
  if (!X || !ss) return fail("dpb_row_sumsq: null argument");
  return launch_rowsumsq(X, rows, N, ss, (hipStream_t)stream);
}

// The perturbed batch and the sampling loop of the reference's local_pca_zt / local_pca_xt (src/utils/utils.py:916-933;
// src/models/ddpm/diffusion.py:396-409): noise.hip
size_t dpb_perturb_scratch_bytes(int B, int64_t n) { return perturb_scratch_bytes(B, n); }

int dpb_perturb_unit(const float* x, const float* noise, uint64_t seed, int64_t first, int B, int64_t n, float norm, float* out, float* noise_out,
                     void* scratch, size_t scratch_bytes, void* stream) {
  if (!x || !out || !scratch) return fail("dpb_perturb_unit: null argument");
  return launch_perturb_unit(x, noise, seed, first, B, n, norm, out, noise_out, scratch, scratch_bytes, (hipStream_t)stream);
}

namespace {
struct LocalPcaScratch { size_t xb = 0, ctxb = 0, part = 0, total = 0; long n_in = 0, n_ctx = 0; };
void local_pca_layout(const dpb_engine* e, LocalPcaScratch& l) {
  l.n_in = (long)e->bufs[e->x_buf].rows * e->x_channels;
  l.n_ctx = e->ctx_buf >= 0 ? (long)e->bufs[e->ctx_buf].rows * e->bufs[e->ctx_buf].Cv : 0;
  ScratchLayout s;
  l.xb = s.take((size_t)e->maxB * l.n_in * sizeof(float));
  l.ctxb = s.take((size_t)e->maxB * l.n_ctx * sizeof(float));
  l.part = s.take(perturb_scratch_bytes(e->maxB, l.n_in));
  l.total = s.off;
}
}  // namespace

size_t dpb_local_pca_scratch_bytes(const dpb_engine* e) {
  LocalPcaScratch l;
  if (e) local_pca_layout(e, l);
  return l.total;
}

int dpb_local_pca_sample(dpb_engine* e, const float* x, float t, const float* ctx, int upto_buf, int channels, const float* noise, uint64_t seed,
                         int64_t first, int64_t count, float* H, void* scratch, size_t scratch_bytes) {
  if (!e || !x || !H || !scratch) return fail("dpb_local_pca_sample: null argument");
  e->cur_batch = 0;                                // as dpb_forward: whatever happens below, the primal state is gone
  if (count < 1 || first < 0 || first > INT64_MAX - count) return fail("dpb_local_pca_sample: first=%lld count=%lld invalid", (long long)first, (long long)count);
  if (upto_buf < 0 || upto_buf >= (int)e->bufs.size() || e->producer[upto_buf] < 0) return fail("invalid upto buffer %d", upto_buf);
  if (channels < 1 || channels > e->bufs[upto_buf].C) return fail("bad channel count");
  if (e->ctx_buf >= 0 && !ctx) return fail("this network needs ctx (encoder_hidden_states)");
  LocalPcaScratch l;
  local_pca_layout(e, l);
  if (int r = check_scratch("dpb_local_pca_sample", "dpb_local_pca_scratch_bytes", scratch, scratch_bytes, l.total)) return r;
  char* sc = (char*)scratch;
  float* xb = (float*)(sc + l.xb);
  float* cb = e->ctx_buf >= 0 ? (float*)(sc + l.ctxb) : nullptr;
  const int64_t D = (int64_t)channels * e->bufs[upto_buf].rows;
  for (int b = 0; cb && b < e->maxB; ++b)          // the conditioning of every chunk: max_batch copies, made once
    DPB_CHECK(hipMemcpyAsync(cb + (size_t)b * l.n_ctx, ctx, (size_t)l.n_ctx * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
  int r = 0;
  for (int64_t c0 = 0; c0 < count && !r; c0 += e->maxB) {
    const int B = (int)std::min<int64_t>(e->maxB, count - c0);
    r = launch_perturb_unit(x, noise ? noise + c0 * l.n_in : nullptr, seed, first + c0, B, l.n_in, 1.f, xb, nullptr, sc + l.part,
                            l.total - l.part, e->stream);
    Forward f;
    f.stash = false; f.temb_resident = c0 > 0;     // same t as the chunk before: its embedding is still in P(temb_buf)
    if (!r) r = forward_pass(e, xb, B, t, cb, upto_buf, channels, H + c0 * D, f);
  }
  return r;
}

// The parallel-h edit chain (reference src/modules/edit.py:1202-1229, :1470-1497): chain.hip between the engine's own passes
size_t dpb_direction_step_scratch_bytes(int64_t n, int64_t N) { return direction_step_scratch_bytes(n, N); }

int dpb_direction_step(const float* W, const float* x, float* x_out, float* vk, const float* step, float sega_sigma, int64_t n, int64_t N, double* stats,
                       void* scratch, size_t scratch_bytes, void* stream) {
  if (!W || !x || !x_out || !step || !stats || !scratch) return fail("dpb_direction_step: null argument");
  return launch_direction_step(W, x, x_out, vk, step, sega_sigma, n, N, stats, scratch, scratch_bytes, (hipStream_t)stream);
}

int dpb_shift_stats(const float* h, const float* h0, const float* u, int nu, const int32_t* dir, const float* sign, int64_t n, int64_t D, double* out,
                    void* stream) {
  if (!h || !h0 || !u || !dir || !sign || !out) return fail("dpb_shift_stats: null argument");
  return launch_shift_stats(h, h0, u, nu, dir, sign, n, D, out, (hipStream_t)stream);
}

namespace {
struct ChainScratch { size_t W = 0, cot = 0, h = 0, h0 = 0, part = 0, total = 0; long n_in = 0, n_h = 0; };
bool chain_layout(const dpb_engine* e, int tap, int n, ChainScratch& l) {
  if (!e || tap < 0 || tap >= (int)e->bufs.size() || n < 1) return false;
  l.n_in = (long)e->bufs[e->x_buf].rows * e->x_channels;
  l.n_h = (long)e->bufs[tap].rows * e->bufs[tap].Cv;
  ScratchLayout s;
  l.W = s.take((size_t)n * l.n_in * sizeof(float));
  l.cot = s.take((size_t)n * l.n_h * sizeof(float));
  l.h = s.take((size_t)n * l.n_h * sizeof(float));
  l.h0 = s.take((size_t)n * l.n_h * sizeof(float));
  l.part = s.take(direction_step_scratch_bytes(n, l.n_in));
  l.total = s.off;
  return true;
}
}  // namespace

size_t dpb_inv_jac_chain_scratch_bytes(const dpb_engine* e, int tap_buf, int n) {
  ChainScratch l;
  return chain_layout(e, tap_buf, n, l) ? l.total : 0;
}

int dpb_inv_jac_chain(dpb_engine* e, int tap_buf, const float* x, int n, const float* t, const float* ctx, const float* u, int nu, const int32_t* dir,
                      const float* sign, const float* step, int steps, float sega_sigma, int final_shift, float* states, float* vk, double* stats,
                      double* shift, void* scratch, size_t scratch_bytes) {
  if (!e || !x || !t || !u || !dir || !sign || !step || !states || !stats || !shift || !scratch) return fail("dpb_inv_jac_chain: null argument");
  e->cur_batch = 0;                                // as dpb_forward: whatever happens below, the primal state is gone
  if (!e->ws) return fail("workspace not set (dpb_engine_set_workspace)");
  const int cap = std::min(e->maxB, e->maxT);
  if (n < 1 || n > cap) return fail("dpb_inv_jac_chain: n=%d chains outside [1,%d] (min of max_batch and max_tangents)", n, cap);
  if (steps < 1) return fail("dpb_inv_jac_chain: steps=%d < 1", steps);
  if (int r = check_dirs("dpb_inv_jac_chain", n, nu, 0, dir, {{"sign", sign}, {"step", step}})) return r;
  if (std::isnan(sega_sigma)) return fail("dpb_inv_jac_chain: sega_sigma is NaN");
  const float* tv;
  if (int r = check_timesteps(e, n, t, &tv)) return r;
  if (int r = check_chain_tap(e, "dpb_inv_jac_chain", tap_buf)) return r;
  if (e->ctx_buf >= 0 && !ctx) return fail("this network needs ctx (encoder_hidden_states)");
  ChainScratch l;
  chain_layout(e, tap_buf, n, l);
  if (int r = check_scratch("dpb_inv_jac_chain", "dpb_inv_jac_chain_scratch_bytes", scratch, scratch_bytes, l.total)) return r;
  char* sc = (char*)scratch;
  float *Wb = (float*)(sc + l.W), *cot = (float*)(sc + l.cot), *hb = (float*)(sc + l.h), *h0 = (float*)(sc + l.h0);
  const Buf& bt = e->bufs[tap_buf];
  const size_t row = (size_t)n * l.n_in;
  CallTotals tot(e);
  if (states != x) DPB_CHECK(hipMemcpyAsync(states, x, row * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
  // the tap activation of the pass just run, as fp32 NCHW, and its shift statistics against the copy kept from step 0
  auto shift_of = [&](int j) -> int {
    float* dst = j == 0 ? h0 : hb;
    if (int r = launch_nhwc_to_nchw(e->dtype, e->P(tap_buf), dst, n, bt.Cv, bt.rows, bt.C, e->stream)) return r;
    return launch_shift_stats(dst, h0, u, nu, dir, sign, n, l.n_h, shift + (size_t)j * n * 2, e->stream);
  };
  int r = 0;
  for (int j = 0; j < steps && !r; ++j) {
    const float* xj = states + (size_t)j * row;
    Forward f;
    f.temb_resident = j > 0;                        // same timesteps as the step before: their embeddings are still in P(temb_buf), no upload, no sync
    r = primal_pass(e, xj, n, t[0], ctx, tap_buf, f, tv);
    tot.add();
    if (!r) r = shift_of(j);
    if (!r) r = launch_gather_cotangents(u, nu, dir, sign, n, l.n_h, cot, e->stream);
    if (!r) r = vjp_pass(e, e->x_buf, tap_buf, cot, n, Wb);
    tot.add();
    if (!r) r = launch_direction_step(Wb, xj, states + (size_t)(j + 1) * row, vk ? vk + (size_t)j * row : nullptr, step, sega_sigma, n, l.n_in,
                                      stats + (size_t)j * n * 4, sc + l.part, l.total - l.part, e->stream);
  }
  if (!r && final_shift) {
    Forward f;
    f.stash = false; f.temb_resident = true;
    r = primal_pass(e, states + (size_t)steps * row, n, t[0], ctx, tap_buf, f, tv);
    tot.add();
    if (!r) r = shift_of(steps);
  } else if (!r) {
    DPB_CHECK(hipMemsetAsync(shift + (size_t)steps * n * 2, 0xff, (size_t)n * 2 * sizeof(double), e->stream));   // all bits set: a NaN
  }
  return tot.close(r);
}

// The least-squares inverse of the Jacobian and the newton-h chain: cgls.hip between the engine's tangent and adjoint passes
size_t dpb_cgls_init_scratch_bytes(int64_t R, int64_t N, int64_t D) { return cgls_scratch_bytes(R, N, D); }
size_t dpb_cgls_h_step_scratch_bytes(int64_t R, int64_t N, int64_t D) { return cgls_scratch_bytes(R, N, D); }
size_t dpb_cgls_x_step_scratch_bytes(int64_t R, int64_t N, int64_t D) { return cgls_scratch_bytes(R, N, D); }

int dpb_cgls_init(const float* c, const float* w0, float* delta, float* r, float* p, double* state, double* hist, double mu_abs, double mu_rel,
                  double tol, int64_t R, int64_t N, int64_t D, void* scratch, size_t scratch_bytes, void* stream) {
  if (!c || !w0 || !delta || !r || !p || !state || !hist || !scratch) return fail("dpb_cgls_init: null argument");
  return launch_cgls_init(c, w0, delta, r, p, state, hist, mu_abs, mu_rel, tol, R, N, D, scratch, scratch_bytes, (hipStream_t)stream);
}

int dpb_cgls_h_step(const float* q, float* delta, float* r, float* p, double* state, double* hist, int64_t R, int64_t N, int64_t D, void* scratch,
                    size_t scratch_bytes, void* stream) {
  if (!q || !delta || !r || !p || !state || !hist || !scratch) return fail("dpb_cgls_h_step: null argument");
  return launch_cgls_h_step(q, delta, r, p, state, hist, R, N, D, scratch, scratch_bytes, (hipStream_t)stream);
}

int dpb_cgls_x_step(const float* w, float* delta, float* r, float* p, double* state, double* hist, double tol, int64_t R, int64_t N, int64_t D,
                    void* scratch, size_t scratch_bytes, void* stream) {
  if (!w || !delta || !r || !p || !state || !hist || !scratch) return fail("dpb_cgls_x_step: null argument");
  return launch_cgls_x_step(w, delta, r, p, state, hist, tol, R, N, D, scratch, scratch_bytes, (hipStream_t)stream);
}

int dpb_newton_residual(const float* h0, const float* h, const float* u, int nu, const int32_t* dir, const float* sign, const float* scale, double frac,
                        int64_t n, int64_t D, float* res, void* stream) {
  if (!h0 || !h || !u || !dir || !sign || !scale || !res) return fail("dpb_newton_residual: null argument");
  return launch_newton_residual(h0, h, u, nu, dir, sign, scale, frac, n, D, res, (hipStream_t)stream);
}

int dpb_newton_update(const float* x, const float* delta, const double* state, double radius, float* x_out, double* step_stats, int64_t n, int64_t N,
                      void* stream) {
  if (!x || !delta || !state || !x_out || !step_stats) return fail("dpb_newton_update: null argument");
  return launch_newton_update(x, delta, state, radius, x_out, step_stats, n, N, (hipStream_t)stream);
}

namespace {
// the solver's working set for nt rows: w = J^T r, q = J p, the residual r, the search direction p, the per-row state and the slice sums
struct LstsqScratch { size_t w = 0, q = 0, r = 0, p = 0, state = 0, part = 0, part_bytes = 0, total = 0; long n_in = 0, n_h = 0; };
void lstsq_take(const dpb_engine* e, int tap, int nt, ScratchLayout& s, LstsqScratch& l) {
  l.n_in = (long)e->bufs[e->x_buf].rows * e->x_channels;
  l.n_h = (long)e->bufs[tap].rows * e->bufs[tap].Cv;
  l.w = s.take((size_t)nt * l.n_in * sizeof(float));
  l.q = s.take((size_t)nt * l.n_h * sizeof(float));
  l.r = s.take((size_t)nt * l.n_h * sizeof(float));
  l.p = s.take((size_t)nt * l.n_in * sizeof(float));
  l.state = s.take((size_t)nt * 8 * sizeof(double));
  l.part_bytes = cgls_scratch_bytes(nt, l.n_in, l.n_h);
  l.part = s.take(l.part_bytes);
  l.total = s.off;
}
bool lstsq_layout(const dpb_engine* e, int tap, int nt, LstsqScratch& l) {
  if (!e || tap < 0 || tap >= (int)e->bufs.size() || nt < 1) return false;
  ScratchLayout s;
  lstsq_take(e, tap, nt, s, l);
  return true;
}

int check_solver_scalars(const char* who, double mu_abs, double mu_rel, double tol, int iters) {
  if (!(mu_abs >= 0.0) || !std::isfinite(mu_abs)) return fail("%s: mu_abs=%g must be finite and not negative", who, mu_abs);
  if (!(mu_rel >= 0.0) || !std::isfinite(mu_rel)) return fail("%s: mu_rel=%g must be finite and not negative", who, mu_rel);
  if (!(tol >= 0.0) || !std::isfinite(tol)) return fail("%s: tol=%g must be finite and not negative", who, tol);
  if (iters < 0) return fail("%s: iters=%d < 0", who, iters);
  return 0;
}

// The inner solve on the primal state of the last pass: one adjoint pass for w0 = J^T c, then iters rounds of tangent pass, h-step, adjoint pass,
// x-step; nothing between them touches the host.  r: the residual rows (the caller's or the scratch's); fl / gb: the passes' flops and bytes.
int lstsq_solve(dpb_engine* e, int tap, const float* c, int nt, double mu_abs, double mu_rel, double tol, int iters, float* delta, float* r, double* hist,
                char* sc, const LstsqScratch& l, double& fl, double& gb) {
  float *w = (float*)(sc + l.w), *q = (float*)(sc + l.q), *p = (float*)(sc + l.p);
  double* state = (double*)(sc + l.state);
  void* part = sc + l.part;
  if (int rc = vjp_pass(e, e->x_buf, tap, c, nt, w)) return rc;
  fl += e->flops; gb += e->gbytes;
  if (int rc = launch_cgls_init(c, w, delta, r, p, state, hist, mu_abs, mu_rel, tol, nt, l.n_in, l.n_h, part, l.part_bytes, e->stream)) return rc;
  for (int i = 1; i <= iters; ++i) {
    double* hi = hist + (size_t)i * nt * 4;
    if (int rc = jvp_pass(e, e->x_buf, tap, p, nt, q)) return rc;
    fl += e->flops; gb += e->gbytes;
    if (int rc = launch_cgls_h_step(q, delta, r, p, state, hi, nt, l.n_in, l.n_h, part, l.part_bytes, e->stream)) return rc;
    if (int rc = vjp_pass(e, e->x_buf, tap, r, nt, w)) return rc;
    fl += e->flops; gb += e->gbytes;
    if (int rc = launch_cgls_x_step(w, delta, r, p, state, hi, tol, nt, l.n_in, l.n_h, part, l.part_bytes, e->stream)) return rc;
  }
  return 0;
}
}  // namespace

size_t dpb_jac_lstsq_scratch_bytes(const dpb_engine* e, int tap_buf, int nt) {
  LstsqScratch l;
  return lstsq_layout(e, tap_buf, nt, l) ? l.total : 0;
}

int dpb_jac_lstsq(dpb_engine* e, int tap_buf, const float* c, int nt, double mu_abs, double mu_rel, double tol, int iters, float* delta, float* resid,
                  double* hist, void* scratch, size_t scratch_bytes) {
  if (!e || !c || !delta || !hist || !scratch) return fail("dpb_jac_lstsq: null argument");
  if (int r = check_solver_scalars("dpb_jac_lstsq", mu_abs, mu_rel, tol, iters)) return r;
  if (int r = check_pass(e, e->x_buf, tap_buf, nt)) return r;
  if ((uintptr_t)hist & 7) return fail("dpb_jac_lstsq: hist must be 8-byte aligned");
  LstsqScratch l;
  lstsq_layout(e, tap_buf, nt, l);
  if (int r = check_scratch("dpb_jac_lstsq", "dpb_jac_lstsq_scratch_bytes", scratch, scratch_bytes, l.total)) return r;
  const long at = launch_count;                     // the sub-passes' LaunchSpans overwrite n_launch as they go: the assignment at the end is what counts
  double fl = 0, gb = 0;
  char* sc = (char*)scratch;
  const int r = lstsq_solve(e, tap_buf, c, nt, mu_abs, mu_rel, tol, iters, delta, resid ? resid : (float*)(sc + l.r), hist, sc, l, fl, gb);
  e->n_launch = launch_count - at; e->flops = fl; e->gbytes = gb;
  return r;
}

namespace {
struct NewtonScratch { size_t h = 0, h0 = 0, res = 0, delta = 0, total = 0; LstsqScratch ls; };
bool newton_layout(const dpb_engine* e, int tap, int n, NewtonScratch& l) {
  if (!e || tap < 0 || tap >= (int)e->bufs.size() || n < 1) return false;
  ScratchLayout s;
  lstsq_take(e, tap, n, s, l.ls);
  l.h = s.take((size_t)n * l.ls.n_h * sizeof(float));
  l.h0 = s.take((size_t)n * l.ls.n_h * sizeof(float));
  l.res = s.take((size_t)n * l.ls.n_h * sizeof(float));
  l.delta = s.take((size_t)n * l.ls.n_in * sizeof(float));
  l.total = s.off;
  return true;
}
}  // namespace

size_t dpb_newton_h_chain_scratch_bytes(const dpb_engine* e, int tap_buf, int n) {
  NewtonScratch l;
  return newton_layout(e, tap_buf, n, l) ? l.total : 0;
}

int dpb_newton_h_chain(dpb_engine* e, int tap_buf, const float* x, int n, const float* t, const float* ctx, const float* u, int nu, const int32_t* dir,
                       const float* sign, const float* scale, int steps, int iters, double mu_abs, double mu_rel, double tol, double radius,
                       int final_shift, float* states, double* hist, double* step_stats, double* shift, void* scratch, size_t scratch_bytes) {
  if (!e || !x || !t || !u || !dir || !sign || !scale || !states || !hist || !step_stats || !shift || !scratch)
    return fail("dpb_newton_h_chain: null argument");
  e->cur_batch = 0;                                // as dpb_forward: whatever happens below, the primal state is gone
  if (!e->ws) return fail("workspace not set (dpb_engine_set_workspace)");
  const int cap = std::min(e->maxB, e->maxT);
  if (n < 1 || n > cap) return fail("dpb_newton_h_chain: n=%d chains outside [1,%d] (min of max_batch and max_tangents)", n, cap);
  if (steps < 1) return fail("dpb_newton_h_chain: steps=%d < 1", steps);
  if (int r = check_dirs("dpb_newton_h_chain", n, nu, 0, dir, {{"sign", sign}, {"scale", scale}})) return r;
  if (int r = check_solver_scalars("dpb_newton_h_chain", mu_abs, mu_rel, tol, iters)) return r;
  if (!(radius >= 0.0) || !std::isfinite(radius)) return fail("dpb_newton_h_chain: radius=%g must be finite and not negative (0: no clamp)", radius);
  const float* tv;
  if (int r = check_timesteps(e, n, t, &tv)) return r;
  if (int r = check_chain_tap(e, "dpb_newton_h_chain", tap_buf)) return r;
  if (e->ctx_buf >= 0 && !ctx) return fail("this network needs ctx (encoder_hidden_states)");
  if ((uintptr_t)hist & 7 || (uintptr_t)step_stats & 7 || (uintptr_t)shift & 7) return fail("dpb_newton_h_chain: hist, step_stats and shift must be 8-byte aligned");
  NewtonScratch l;
  newton_layout(e, tap_buf, n, l);
  if (int r = check_scratch("dpb_newton_h_chain", "dpb_newton_h_chain_scratch_bytes", scratch, scratch_bytes, l.total)) return r;
  char* sc = (char*)scratch;
  float *hb = (float*)(sc + l.h), *h0 = (float*)(sc + l.h0), *res = (float*)(sc + l.res), *delta = (float*)(sc + l.delta);
  const Buf& bt = e->bufs[tap_buf];
  const long n_in = l.ls.n_in, n_h = l.ls.n_h;
  const size_t row = (size_t)n * n_in;
  CallTotals tot(e);
  if (states != x) DPB_CHECK(hipMemcpyAsync(states, x, row * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
  // the tap activation of the pass just run, as fp32 NCHW, and its shift statistics against the copy kept from step 0
  auto shift_of = [&](int j) -> int {
    float* dst = j == 0 ? h0 : hb;
    if (int r = launch_nhwc_to_nchw(e->dtype, e->P(tap_buf), dst, n, bt.Cv, bt.rows, bt.C, e->stream)) return r;
    return launch_shift_stats(dst, h0, u, nu, dir, sign, n, n_h, shift + (size_t)j * n * 2, e->stream);
  };
  int r = 0;
  for (int j = 0; j < steps && !r; ++j) {
    const float* xj = states + (size_t)j * row;
    Forward f;
    f.temb_resident = j > 0;                        // same timesteps as the step before: their embeddings are still in P(temb_buf), no upload, no sync
    r = primal_pass(e, xj, n, t[0], ctx, tap_buf, f, tv);
    tot.add();
    if (!r) r = shift_of(j);
    if (!r) r = launch_newton_residual(h0, j == 0 ? h0 : hb, u, nu, dir, sign, scale, (double)(j + 1) / (double)steps, n, n_h, res, e->stream);
    if (!r) r = lstsq_solve(e, tap_buf, res, n, mu_abs, mu_rel, tol, iters, delta, (float*)(sc + l.ls.r), hist + (size_t)j * (iters + 1) * n * 4, sc, l.ls,
                            tot.fl, tot.gb);
    if (!r) r = launch_newton_update(xj, delta, (const double*)(sc + l.ls.state), radius, states + (size_t)(j + 1) * row, step_stats + (size_t)j * n * 4, n,
                                     n_in, e->stream);
  }
  if (!r && final_shift) {
    Forward f;
    f.stash = false; f.temb_resident = true;
    r = primal_pass(e, states + (size_t)steps * row, n, t[0], ctx, tap_buf, f, tv);
    tot.add();
    if (!r) r = shift_of(steps);
  } else if (!r) {
    DPB_CHECK(hipMemsetAsync(shift + (size_t)steps * n * 2, 0xff, (size_t)n * 2 * sizeof(double), e->stream));   // all bits set: a NaN
  }
  return tot.close(r);
}

// The h-space guidance edit (hguide.hip between the engine's grouped passes): dpb_ddim_step_asym and the device DDIM chain
size_t dpb_ddim_step_asym_scratch_bytes(int64_t n, int64_t N) { return ddim_step_asym_scratch_bytes(n, N); }

int dpb_ddim_step_asym(const float* x, const float* e, const float* e_s, float* out, float* x0, int64_t n, int64_t N, float alpha_t, float alpha_next,
                       float gP, float gD, double* stats, void* scratch, size_t scratch_bytes, void* stream) {
  if (!x || !e || !e_s || !out || !stats || !scratch) return fail("dpb_ddim_step_asym: null argument");
  return launch_ddim_step_asym(x, e, e_s, out, x0, n, N, alpha_t, alpha_next, gP, gD, stats, scratch, scratch_bytes, (hipStream_t)stream);
}

namespace {
struct HguideScratch { size_t temb = 0, eps = 0, part = 0, total = 0; long n_in = 0, temb_c = 0; };
bool hguide_layout(const dpb_engine* e, int n, int steps, HguideScratch& l) {
  if (!e || n < 1 || steps < 1) return false;
  l.n_in = (long)e->bufs[e->x_buf].rows * e->x_channels;
  l.temb_c = e->temb_buf >= 0 ? e->bufs[e->temb_buf].C : 0;
  ScratchLayout s;
  l.temb = s.take((size_t)steps * l.temb_c * sizeof(float));
  l.eps = s.take((size_t)2 * n * l.n_in * sizeof(float));
  l.part = s.take(ddim_step_asym_scratch_bytes(n, l.n_in));
  l.total = s.off;
  return true;
}
}  // namespace

size_t dpb_hguide_chain_scratch_bytes(const dpb_engine* e, int n, int steps) {
  HguideScratch l;
  return hguide_layout(e, n, steps, l) ? l.total : 0;
}

int dpb_hguide_chain(dpb_engine* e, int tap_buf, int eps_buf, const float* x, int n, const float* t, const float* alpha_t, const float* alpha_next,
                     const float* ctx, const float* u, int nu, const int32_t* dir, const float* scale, float gP, float gD, int steps, float* states,
                     double* delta, void* scratch, size_t scratch_bytes) {
  if (!e || !x || !t || !alpha_t || !alpha_next || !u || !dir || !scale || !states || !delta || !scratch) return fail("dpb_hguide_chain: null argument");
  e->cur_batch = 0;                                // as dpb_forward: whatever happens below, the primal state is gone
  if (!e->ws) return fail("workspace not set (dpb_engine_set_workspace)");
  if (n < 1 || 2 * (long)n > e->maxB) return fail("dpb_hguide_chain: n=%d chains: a plain and a shifted row each, 2n outside [2,%d] (max_batch)", n, e->maxB);
  if (steps < 1) return fail("dpb_hguide_chain: steps=%d < 1", steps);
  if (int r = check_dirs("dpb_hguide_chain", n, nu, 0, dir, {{"scale", scale}})) return r;
  if (!isfinite(gP) || !isfinite(gD)) return fail("dpb_hguide_chain: gP=%g, gD=%g: not finite", gP, gD);
  for (int j = 0; j < steps; ++j) {
    if (!isfinite(t[j])) return fail("dpb_hguide_chain: t[%d] is not finite", j);
    if (!(alpha_t[j] > 0.f && alpha_t[j] <= 1.f) || !(alpha_next[j] > 0.f && alpha_next[j] <= 1.f))
      return fail("dpb_hguide_chain: step %d: alpha_t=%g and alpha_next=%g must lie in (0, 1]", j, alpha_t[j], alpha_next[j]);
  }
  if (int r = check_chain_tap(e, "dpb_hguide_chain", tap_buf)) return r;
  if (int r = check_pair(e, tap_buf, eps_buf, FOR_FORWARD)) return r;
  const Buf& be = e->bufs[eps_buf];
  if (be.Cv != e->x_channels || be.rows != e->bufs[e->x_buf].rows)
    return fail("dpb_hguide_chain: eps buffer %d is [%d][%d], the input is [%d][%d]: a DDIM step needs the two to agree", eps_buf, be.Cv, be.rows,
                e->x_channels, e->bufs[e->x_buf].rows);
  if (e->ctx_buf >= 0 && !ctx) return fail("this network needs ctx (encoder_hidden_states)");
  HguideScratch l;
  hguide_layout(e, n, steps, l);
  if (int r = check_scratch("dpb_hguide_chain", "dpb_hguide_chain_scratch_bytes", scratch, scratch_bytes, l.total)) return r;
  char* sc = (char*)scratch;
  float *temb = (float*)(sc + l.temb), *eps = (float*)(sc + l.eps);
  const size_t row = (size_t)n * l.n_in;
  CallTotals tot(e);
  // rows 0 .. n-1: the plain net; rows n .. 2n-1: the chains' shifts
  std::vector<int32_t> dirs(2 * n, -1);
  std::vector<float> scales(2 * n, 0.f);
  for (int b = 0; b < n; ++b) { dirs[n + b] = dir[b]; scales[n + b] = scale[b]; }
  if (e->temb_buf >= 0) {
    // the sinusoid rows of ALL the steps in one copy: the call's one host synchronisation (emb is a host temporary)
    std::vector<float> emb((size_t)steps * l.temb_c, 0.f);
    for (int j = 0; j < steps; ++j) temb_row(e, t[j], emb.data() + (size_t)j * l.temb_c);
    DPB_CHECK(hipMemcpyAsync(temb, emb.data(), emb.size() * sizeof(float), hipMemcpyHostToDevice, e->stream));
    DPB_CHECK(hipStreamSynchronize(e->stream));
  }
  if (states != x) DPB_CHECK(hipMemcpyAsync(states, x, row * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
  int r = 0;
  for (int j = 0; j < steps && !r; ++j) {
    const float* xj = states + (size_t)j * row;
    if (e->temb_buf >= 0)
      r = launch_nchw_to_nhwc(e->dtype, temb + (size_t)j * l.temb_c, e->P(e->temb_buf), 1, (int)l.temb_c, 1, (int)l.temb_c, e->stream);
    Forward f;
    f.stash = false; f.temb_resident = true;       // step j's row was moved into P(temb_buf) on the device just now: no upload, no sync
    f.seed = tap_buf; f.u = u; f.dir = dirs.data(); f.scale = scales.data(); f.xbatch = n; f.groups = 2;
    if (!r) r = primal_pass(e, xj, 2 * n, t[j], ctx, eps_buf, f);
    tot.add();
    if (!r) r = launch_nhwc_to_nchw(e->dtype, e->P(eps_buf), eps, 2 * n, be.Cv, be.rows, be.C, e->stream);
    if (!r) r = launch_ddim_step_asym(xj, eps, eps + row, states + (size_t)(j + 1) * row, nullptr, n, l.n_in, alpha_t[j], alpha_next[j], gP, gD,
                                      delta + (size_t)j * n * 2, sc + l.part, l.total - l.part, e->stream);
  }
  return tot.close(r);
}

// Pullback geodesics between two latents (geodesic_chain.hip between the engine's own passes): the two kernels and the device energy chain
size_t dpb_geodesic_cotangents_scratch_bytes(int64_t m, int64_t D) { return geodesic_cotangents_scratch_bytes(m, D); }

int dpb_geodesic_cotangents(const float* h, float* cot, double* seg, double* csq, int64_t m, int64_t D, void* scratch, size_t scratch_bytes, void* stream) {
  if (!h || !cot || !seg || !scratch) return fail("dpb_geodesic_cotangents: null argument");
  return launch_geodesic_cotangents(h, cot, seg, csq, m, D, scratch, scratch_bytes, (hipStream_t)stream);
}

size_t dpb_geodesic_update_scratch_bytes(int64_t m, int64_t N) { return geodesic_update_scratch_bytes(m, N); }

int dpb_geodesic_update(const float* P, const float* W, float* P_out, float eta, float lambda, int64_t m, int64_t N, double* stats, double* xseg,
                        void* scratch, size_t scratch_bytes, void* stream) {
  if (!P || !W || !P_out || !stats || !xseg || !scratch) return fail("dpb_geodesic_update: null argument");
  return launch_geodesic_update(P, W, P_out, eta, lambda, m, N, stats, xseg, scratch, scratch_bytes, (hipStream_t)stream);
}

namespace {
struct GeodesicScratch { size_t h = 0, cot = 0, W = 0, x2 = 0, ctx2 = 0, part = 0, total = 0, part_bytes = 0; long n_in = 0, n_h = 0, n_ctx = 0; };
bool geodesic_layout(const dpb_engine* e, int tap, int m, GeodesicScratch& l) {
  if (!e || tap < 0 || tap >= (int)e->bufs.size() || m < 1) return false;
  l.n_in = (long)e->bufs[e->x_buf].rows * e->x_channels;
  l.n_h = (long)e->bufs[tap].rows * e->bufs[tap].Cv;
  l.n_ctx = e->ctx_buf >= 0 ? (long)e->bufs[e->ctx_buf].rows * e->bufs[e->ctx_buf].Cv : 0;
  l.part_bytes = std::max(geodesic_cotangents_scratch_bytes(m, l.n_h), geodesic_update_scratch_bytes(m, l.n_in));
  ScratchLayout s;
  l.h = s.take((size_t)(m + 2) * l.n_h * sizeof(float));
  l.cot = s.take((size_t)m * l.n_h * sizeof(float));
  l.W = s.take((size_t)m * l.n_in * sizeof(float));
  l.x2 = s.take((size_t)2 * l.n_in * sizeof(float));
  l.ctx2 = s.take((size_t)2 * l.n_ctx * sizeof(float));
  l.part = s.take(l.part_bytes);
  l.total = s.off;
  return true;
}
}  // namespace

size_t dpb_geodesic_chain_scratch_bytes(const dpb_engine* e, int tap_buf, int m) {
  GeodesicScratch l;
  return geodesic_layout(e, tap_buf, m, l) ? l.total : 0;
}

int dpb_geodesic_chain(dpb_engine* e, int tap_buf, const float* P, int m, float t, const float* ctx, float eta, float lambda, int iters, int final_energy,
                       float* curves, double* seg_h, double* seg_x, double* stats, double* csq, void* scratch, size_t scratch_bytes) {
  if (!e || !P || !curves || !seg_h || !seg_x || !stats || !scratch) return fail("dpb_geodesic_chain: null argument");
  e->cur_batch = 0;                                // as dpb_forward: whatever happens below, the primal state is gone
  if (!e->ws) return fail("workspace not set (dpb_engine_set_workspace)");
  if (e->maxB < 2) return fail("dpb_geodesic_chain: max_batch=%d: the two end points run as one batch of 2", e->maxB);
  const int cap = std::min(e->maxB, e->maxT);
  if (m < 1 || m > cap) return fail("dpb_geodesic_chain: m=%d interior points outside [1,%d] (min of max_batch and max_tangents)", m, cap);
  if (iters < 1) return fail("dpb_geodesic_chain: iters=%d < 1", iters);
  if (!isfinite(t) || !isfinite(eta) || !isfinite(lambda) || lambda < 0.f)
    return fail("dpb_geodesic_chain: t=%g, eta=%g and lambda=%g must be finite, lambda >= 0", t, eta, lambda);
  if (int r = check_chain_tap(e, "dpb_geodesic_chain", tap_buf)) return r;
  if (e->ctx_buf >= 0 && !ctx) return fail("this network needs ctx (encoder_hidden_states)");
  GeodesicScratch l;
  geodesic_layout(e, tap_buf, m, l);
  if (int r = check_scratch("dpb_geodesic_chain", "dpb_geodesic_chain_scratch_bytes", scratch, scratch_bytes, l.total)) return r;
  char* sc = (char*)scratch;
  float *hb = (float*)(sc + l.h), *cot = (float*)(sc + l.cot), *Wb = (float*)(sc + l.W), *x2 = (float*)(sc + l.x2), *ctx2 = e->ctx_buf >= 0 ? (float*)(sc + l.ctx2) : nullptr;
  const float* ctx_in = ctx2 ? ctx + l.n_ctx : nullptr;      // the conditioning of the interior rows
  const Buf& bt = e->bufs[tap_buf];
  const size_t row = (size_t)(m + 2) * l.n_in, last = (size_t)(m + 1) * l.n_in;
  CallTotals tot(e);
  if (curves != P) DPB_CHECK(hipMemcpyAsync(curves, P, row * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
  // The end points: one pass at batch 2 (it uploads the time embedding: the call's one host synchronisation), their tap activations kept as fp32 NCHW in
  // rows 0 and m + 1 of the [m + 2][N_h] block for the whole call
  DPB_CHECK(hipMemcpyAsync(x2, P, (size_t)l.n_in * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
  DPB_CHECK(hipMemcpyAsync(x2 + l.n_in, P + last, (size_t)l.n_in * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
  if (ctx2) {
    DPB_CHECK(hipMemcpyAsync(ctx2, ctx, (size_t)l.n_ctx * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
    DPB_CHECK(hipMemcpyAsync(ctx2 + l.n_ctx, ctx + (size_t)(m + 1) * l.n_ctx, (size_t)l.n_ctx * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
  }
  Forward f0;
  f0.stash = false;
  int r = primal_pass(e, x2, 2, t, ctx2, tap_buf, f0);
  tot.add();
  const size_t sample = (size_t)bt.rows * bt.C * e->es;      // bytes of one sample of the tap buffer
  if (!r) r = launch_nhwc_to_nchw(e->dtype, e->P(tap_buf), hb, 1, bt.Cv, bt.rows, bt.C, e->stream);
  if (!r) r = launch_nhwc_to_nchw(e->dtype, e->P(tap_buf) + sample, hb + (size_t)(m + 1) * l.n_h, 1, bt.Cv, bt.rows, bt.C, e->stream);
  // the tap activations of the interior rows of `curve` into the middle of the block, then the cotangents and the h-segments of row j
  auto energy_of = [&](const float* curve, int j, bool stash) -> int {
    Forward f;
    f.stash = stash; f.temb_resident = true;       // the end-point pass left this t's embedding in P(temb_buf): no upload, no sync
    int q = primal_pass(e, curve + l.n_in, m, t, ctx_in, tap_buf, f);
    tot.add();
    if (!q) q = launch_nhwc_to_nchw(e->dtype, e->P(tap_buf), hb + l.n_h, m, bt.Cv, bt.rows, bt.C, e->stream);
    if (!q) q = launch_geodesic_cotangents(hb, cot, seg_h + (size_t)j * (m + 1), csq && j < iters ? csq + (size_t)j * m : nullptr, m, l.n_h, sc + l.part,
                                           l.part_bytes, e->stream);
    return q;
  };
  for (int j = 0; j < iters && !r; ++j) {
    const float* cj = curves + (size_t)j * row;
    r = energy_of(cj, j, true);
    if (!r) r = vjp_pass(e, e->x_buf, tap_buf, cot, m, Wb);
    tot.add();
    if (!r) r = launch_geodesic_update(cj, Wb, curves + (size_t)(j + 1) * row, eta, lambda, m, l.n_in, stats + (size_t)j * m * 4,
                                       seg_x + (size_t)j * (m + 1), sc + l.part, l.part_bytes, e->stream);
  }
  if (!r && final_energy) {
    r = energy_of(curves + (size_t)iters * row, iters, false);
    // the x-segments of the last curve: the segment sums of the cotangent kernel (cot = null: nothing else), the chain of the update kernel's xseg
    if (!r) r = launch_geodesic_cotangents(curves + (size_t)iters * row, nullptr, seg_x + (size_t)iters * (m + 1), nullptr, m, l.n_in, sc + l.part, l.part_bytes, e->stream);
  } else if (!r) {
    DPB_CHECK(hipMemsetAsync(seg_h + (size_t)iters * (m + 1), 0xff, (size_t)(m + 1) * sizeof(double), e->stream));   // all bits set: a NaN
    DPB_CHECK(hipMemsetAsync(seg_x + (size_t)iters * (m + 1), 0xff, (size_t)(m + 1) * sizeof(double), e->stream));
  }
  return tot.close(r);
}

static int g_iter_alias = getenv("DPB_ITER_ALIAS") ? atoi(getenv("DPB_ITER_ALIAS")) : 1;   // A/B switch: 0 = convert U out and back in every iteration
static int g_orth_batch = getenv("DPB_ORTH_BATCH") ? atoi(getenv("DPB_ORTH_BATCH")) : 1;   // A/B switch: 0 = re-orthonormalise the samples of a batch one by one
static int g_graph_iterate = 0;      // dpb_debug_set("graph_iterate", 1): replay the power iteration as a captured hipGraph (measurement option)

// The power iteration between seed `src` and `tap`.  Wm: fp32 [B][k][N] staging of W = J^T J V, orth_scratch: B slots of orth_stride bytes
// (the encoder entry point: the engine's workspace; the *_between one: the caller's scratch).
static int iterate_pass(dpb_engine* e, int src, int tap, float* V, float* U, float* s, float* conv, int k, int n_iters, float* Wm, char* orth_scratch,
                        size_t orth_stride) {
  const int B = e->cur_batch;
  const int nt = k * B;
  const long N = (long)e->bufs[src].rows * seed_channels(e, src);
  const long at = launch_count;                     // the sub-passes' LaunchSpans overwrite n_launch as they go: the assignment at the end is what counts
  long replayed = 0;                                // launches of the graph replays, less those counted while the graph was captured (they did not run)
  double fl = 0, gb = 0;
  const bool alias_ok = e->bufs[tap].Cv == e->bufs[tap].C && g_iter_alias;   // (padded tap channels: the conversion kernels zero them, an alias would not)
  auto body = [&](bool want_u) -> int {             // one power iteration: k JVPs, k VJPs, re-orthonormalisation, V <- V_new; no host sync
    // U = J V_prev is an OUTPUT of the last iteration only (utils.py:810): before that the tap's tangent goes straight from T(tap) into the adjoint
    // pass -- no nhwc -> fp32 nchw -> nhwc round trip (two launches per iteration, bitwise the same values)
    const bool keep = alias_ok && !want_u;
    if (int r = jvp_pass(e, src, tap, V, nt, keep ? nullptr : U)) return r;
    fl += e->flops; gb += e->gbytes;
    if (int r = vjp_pass(e, src, tap, keep ? nullptr : U, nt, Wm)) return r;
    fl += e->flops; gb += e->gbytes;
    {                                               // independent k x N re-orthonormalisation per sample, all samples in one set of four launches
      OrthArgs a = orth_args(Wm, V, V, s, conv, orth_scratch, orth_scratch_bytes(k, N), k, N);   // (in place, V is Vprev: see dpb.h)
      a.batch = B; a.stride_w = (long)k * N; a.stride_v = (long)k * N; a.stride_s = k; a.stride_conv = 2; a.scratch_stride = orth_stride;
      if (g_orth_batch) {
        if (int r = launch_orth(a, e->stream)) return r;
      } else {                                      // A/B switch DPB_ORTH_BATCH=0: four launches per sample, as rounds 1-5 (same bits)
        a.batch = 1;
        for (int b = 0; b < B; ++b) {
          if (int r = launch_orth(a, e->stream)) return r;
          a.W += a.stride_w; a.Vprev += a.stride_v; a.V += a.stride_v; a.s += k; a.conv += 2; a.scratch += orth_stride / sizeof(double);
        }
      }
    }
    return 0;
  };
  int it = 0;
  if (g_graph_iterate && !e->profiling && e->stream != 0 && src == e->x_buf) {   // (the captured graph is keyed on the tap alone: encoder entry point only)
    // The launch sequence of an iteration is fixed for fixed (tap, k, batch, buffers): capture it once (after one eager iteration, so that
    // every code object is loaded) and replay it.  Measured on MI355X: no gain -- the stream never runs dry.
    const dpb_engine::GraphKey key{tap, k, B, V, U, s, conv};
    if (!e->gexec || !(key == e->gkey)) {
      if (int r = body(true)) return r;
      ++it;
      if (e->gexec) { (void)hipGraphExecDestroy(e->gexec); e->gexec = nullptr; }
      hipGraph_t g = nullptr;
      const long l0 = launch_count; const double f0 = fl, b0 = gb;
      DPB_CHECK(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
      const int r = body(true);                     // the captured iteration always writes U (it may be the last one replayed)
      const hipError_t ce = hipStreamEndCapture(e->stream, &g);
      e->g_launches = launch_count - l0; e->g_flops = fl - f0; e->g_bytes = gb - b0;
      replayed -= e->g_launches; fl = f0; gb = b0;   // captured, not executed
      if (r) { if (g) (void)hipGraphDestroy(g); return r; }
      DPB_CHECK(ce);
      DPB_CHECK(hipGraphInstantiate(&e->gexec, g, nullptr, nullptr, 0));
      (void)hipGraphDestroy(g);
      e->gkey = key;
    }
    for (; it < n_iters; ++it) {
      DPB_CHECK(hipGraphLaunch(e->gexec, e->stream));
      replayed += e->g_launches; fl += e->g_flops; gb += e->g_bytes;
    }
  }
  for (; it < n_iters; ++it)
    if (int r = body(it == n_iters - 1)) return r;
  e->n_launch = launch_count - at + replayed; e->flops = fl; e->gbytes = gb;
  return 0;
}

int dpb_pullback_iterate(dpb_engine* e, int tap, float* V, float* U, float* s, float* conv, int k, int n_iters) {
  if (!e || !V || !U || !s || !conv) return fail("null argument");
  if (k < 1 || k > ORTH_MAX_RANK) return fail("pca_rank k=%d outside [1,%d]", k, ORTH_MAX_RANK);
  const int B = e->cur_batch;                       // samples advanced together: one weight stream for all of them
  if (int r = check_tap(e, tap, k * (B > 0 ? B : 1))) return r;
  return iterate_pass(e, e->x_buf, tap, V, U, s, conv, k, n_iters, (float*)(e->ws + e->pbW), e->ws + e->orth, e->orth_stride);
}

// scratch of the *_between iteration for `batch` samples: W staging, then one re-orthonormalisation slot per sample
static size_t between_scratch_bytes(const dpb_engine* e, int src, int k, int batch) {
  const long N = (long)e->bufs[src].rows * seed_channels(e, src);
  return align_up((size_t)batch * k * N * sizeof(float)) + (size_t)batch * align_up(orth_scratch_bytes(k, N));
}

size_t dpb_pullback_scratch_bytes(const dpb_engine* e, int src_buf, int k) {
  if (!e || k < 1 || k > ORTH_MAX_RANK || src_buf < 0 || src_buf >= (int)e->bufs.size() || e->bufs[src_buf].kind != DPB_BUF_ACT) return 0;
  return between_scratch_bytes(e, src_buf, k, e->maxB);
}

int dpb_pullback_iterate_between(dpb_engine* e, int src_buf, int dst_buf, float* V, float* U, float* s, float* conv, int k, int n_iters, void* scratch,
                                 size_t scratch_bytes) {
  if (!e || !V || !U || !s || !conv || !scratch) return fail("null argument");
  if (k < 1 || k > ORTH_MAX_RANK) return fail("pca_rank k=%d outside [1,%d]", k, ORTH_MAX_RANK);
  const int B = e->cur_batch;
  if (int r = check_pass(e, src_buf, dst_buf, k * (B > 0 ? B : 1))) return r;
  if ((uintptr_t)scratch % 256) return fail("scratch must be 256-byte aligned");
  const size_t need = between_scratch_bytes(e, src_buf, k, B);
  if (scratch_bytes < need) return fail("scratch of %zu bytes, the iteration needs %zu (dpb_pullback_scratch_bytes)", scratch_bytes, need);
  const long N = (long)e->bufs[src_buf].rows * seed_channels(e, src_buf);
  const size_t wbytes = align_up((size_t)B * k * N * sizeof(float));      // the layout of between_scratch_bytes
  return iterate_pass(e, src_buf, dst_buf, V, U, s, conv, k, n_iters, (float*)scratch, (char*)scratch + wbytes, align_up(orth_scratch_bytes(k, N)));
}

int dpb_ddim_step(const float* x, const float* eps, float* out, float* x0, int64_t n, float a_t, float a_next, void* stream) {
  if (!x || !eps || !out) return fail("null argument");
  return launch_ddim_step(x, eps, out, x0, n, a_t, a_next, (hipStream_t)stream);
}

int dpb_embed_tokens(const int32_t* ids, const void* tok_table, const void* pos_table, int dtype, float* out, int batch, int tokens,
                     int channels, int vocab, void* stream) {
  if (!ids || !tok_table || !pos_table || !out) return fail("null argument");
  if (dtype != DPB_F32 && dtype != DPB_BF16 && dtype != DPB_F16) return fail("bad dtype %d", dtype);
  return launch_embed_tokens(dtype, ids, tok_table, pos_table, out, batch, tokens, channels, vocab, (hipStream_t)stream);
}

int dpb_lincomb(const float* x, const float* y, const float* z, float* out, int64_t n, float a, float b, float c, void* stream) {
  if (!x || !y || !out) return fail("null argument");
  return launch_lincomb(x, y, z, out, n, a, b, c, (hipStream_t)stream);
}

int dpb_engine_profile(dpb_engine* e, int enable) {
  if (!e) return fail("null engine");
  for (auto& p : e->prof) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
  e->prof.clear();
  e->profiling = enable != 0;
  if (e->profiling) {
    // an event pair brackets more than the kernel's execution (event processing, dispatch ramp of the launch it encloses): measure the
    // bracket around a 64-element copy -- a kernel whose own execution is ~1.5 us in rocprofv3's kernel trace -- and subtract the
    // excess from every launch, so the per-launch durations agree with the kernel trace (cross-checked in profiles/)
    hipEvent_t a, b;
    DPB_CHECK(hipEventCreate(&a));
    DPB_CHECK(hipEventCreate(&b));
    float best = 1e9f;
    for (int i = 0; i < 24; ++i) {
      DPB_CHECK(hipEventRecord(a, e->stream));
      if (int r = launch_axpy(e->dtype, e->ws + e->zeros, e->ws + e->zeros, 64, 0, e->stream)) return r;
      DPB_CHECK(hipEventRecord(b, e->stream));
      DPB_CHECK(hipEventSynchronize(b));
      float ms = 0;
      DPB_CHECK(hipEventElapsedTime(&ms, a, b));
      if (i >= 4) best = ms < best ? ms : best;
    }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    best -= 1.5e-3f;
    if (best < 0.f) best = 0.f;
    e->prof_overhead_ms = best < 1e8f ? best : 0.f;
  }
  return 0;
}

int dpb_engine_profile_dump(dpb_engine* e, const char* path) {
  if (!e || !path) return fail("null argument");
  DPB_CHECK(hipStreamSynchronize(e->stream));
  FILE* f = fopen(path, "w");
  if (!f) return fail("cannot open %s", path);
  fprintf(f, "idx,big,gather,M,N,K,Z,us,tflops,raw_us,bracket_overhead_us\n");   // us = raw_us - bracket_overhead_us (calibrated empty-bracket time)
  int i = 0;
  for (auto& p : e->prof) {
    float raw = 0;
    (void)hipEventElapsedTime(&raw, p.a, p.b);
    const float ms = raw > e->prof_overhead_ms ? raw - e->prof_overhead_ms : 0.f;
    fprintf(f, "%d,%d,%d,%d,%d,%d,%d,%.2f,%.2f,%.2f,%.2f\n", i++, p.big, p.gather, p.M, p.N, p.K, p.Z, ms * 1e3, ms > 0 ? p.flops / (ms * 1e-3) / 1e12 : 0.0,
            raw * 1e3, e->prof_overhead_ms * 1e3);
  }
  fclose(f);
  return 0;
}

int dpb_engine_profile_read(dpb_engine* e, int big_tile, int64_t* count, double* total_ms, double* flops) {
  if (!e || !count || !total_ms || !flops) return fail("null argument");
  DPB_CHECK(hipStreamSynchronize(e->stream));
  *count = 0; *total_ms = 0; *flops = 0;
  const bool raw = big_tile >= 1000;                 // kind + 1000: the RAW bracket times (no empty-bracket correction, nothing clamped)
  if (raw) big_tile -= 1000;
  if (big_tile < 0 || big_tile > 12) return fail("dpb_engine_profile_read: kind must be 0..12 or 1000..1012");
  for (auto& p : e->prof) {
    if (p.big != big_tile) continue;
    float ms = 0;
    DPB_CHECK(hipEventElapsedTime(&ms, p.a, p.b));
    if (!raw) ms = ms > e->prof_overhead_ms ? ms - e->prof_overhead_ms : 0.f;
    *count += 1; *total_ms += ms; *flops += p.flops;
  }
  return 0;
}

int dpb_engine_profile_overhead(const dpb_engine* e, double* bracket_overhead_ms) {
  if (!e || !bracket_overhead_ms) return fail("null argument");
  *bracket_overhead_ms = e->prof_overhead_ms;
  return 0;
}

int dpb_debug_set(const char* key, int value) {
  static int tile = 0, splitk = 0, kch = 0;
  if (!key) return fail("null key");
  if (!strcmp(key, "gemm_tile")) tile = value;
  else if (!strcmp(key, "gemm_splitk")) splitk = value;
  else if (!strcmp(key, "gemm_kch")) kch = value;
  else if (!strcmp(key, "gemm_dma_auto")) { gemm_debug_dma_auto(value); return 0; }
  else if (!strcmp(key, "gemm_order")) { gemm_debug_order(value); return 0; }
  else if (!strcmp(key, "p8")) { gemm_debug_p8(value); return 0; }
  else if (!strcmp(key, "halo_loop")) { conv_halo_debug_loop(value); return 0; }
  else if (!strcmp(key, "wres")) { gemm_debug_wres(value); return 0; }
  else if (!strcmp(key, "gn_deterministic")) { gn_debug_deterministic(value); return 0; }
  else if (!strcmp(key, "graph_iterate")) { g_graph_iterate = value; return 0; }
  else if (!strcmp(key, "attn_shared")) { attn_debug_shared(value); return 0; }
  else if (!strcmp(key, "lazy_reduce")) { g_lazy_reduce = value; return 0; }
  else if (!strcmp(key, "ln_fuse")) { g_ln_fuse = value; return 0; }
  else if (!strcmp(key, "cross_primal")) { g_cross_primal = value; return 0; }
  else if (!strcmp(key, "cross_fold")) { g_cross_fold = value; return 0; }
  else if (!strcmp(key, "geglu_fwd")) { g_geglu_fwd = value; return 0; }
  else if (!strcmp(key, "iter_alias")) { g_iter_alias = value; return 0; }
  else if (!strcmp(key, "pga_route")) { pga_debug_route(value); return 0; }
  else return fail("unknown debug key %s", key);
  gemm_debug_set(tile, splitk, kch);
  return 0;
}

int dpb_debug_gemm_plan(int dtype, int M, int N, int K, int conv_hw, int conv_cin, int epilogue, int64_t slab_bytes, int* kind, int* tile,
                        int* splitk) {
  if (!kind || !tile || !splitk) return fail("null argument");
  if (dtype != DPB_F32 && dtype != DPB_BF16 && dtype != DPB_F16) return fail("bad dtype %d", dtype);
  static char dummy[16];                       // the plan only looks at which pointers are set, never through them
  GemmArgs a;
  a.M = M; a.N = N; a.K = K; a.lda = K; a.ldb = K; a.ldc = N;
  a.zeros = dummy;
  if (slab_bytes > 0) { a.slab = (float*)dummy; a.slab_bytes = (size_t)slab_bytes; }
  a.epi = epilogue;
  if (epilogue == EPI_XATT) { a.xatt_p = (const float*)dummy; a.xatt_h = N / 128; a.xatt_lk = 77; a.ldc = 80 * a.xatt_h; a.C = dummy; }   // N = 128 heads
  if (conv_hw > 0) {                           // 3x3, stride 1, pad 1 on conv_hw x conv_hw images of conv_cin channels
    if (conv_cin <= 0 || K != 9 * conv_cin || M % (conv_hw * conv_hw)) return fail("conv plan: K must be 9*cin and M whole images");
    a.gather = GATHER_CONV; a.H = a.W = a.Ho = a.Wo = conv_hw; a.Cin = conv_cin; a.KS = 3; a.stride = 1; a.pad = 1; a.lda = conv_cin;
  }
  const GemmPlan pl = gemm_plan(dtype, a);
  if (!pl.row) return -1;
  *kind = pl.kind; *tile = pl.tile; *splitk = pl.splitk;
  return 0;
}

int dpb_debug_cross_fold(const dpb_engine* e, int index, int64_t* info) {
  if (!e || !info) return fail("null argument");
  int n = 0;
  for (size_t i = 0; i < e->ops.size(); ++i) {
    if (e->ops[i].d.kind != DPB_OP_ATTENTION || !e->plans[e->ops[i].attn].fold_ok) continue;
    if (n++ != index) continue;
    const AttnPlan& p = e->plans[e->ops[i].attn];
    const int64_t v[12] = {(int64_t)i, p.fold_live, p.heads * p.d, p.heads, p.Lq, p.Lk, (int64_t)p.Gt, (int64_t)p.Gk, (int64_t)p.F, (int64_t)p.Fk, (int64_t)p.Pf, (int64_t)e->S1};
    memcpy(info, v, sizeof(v));
    return 0;
  }
  return fail("dpb_debug_cross_fold: the tape has %d layers that can take the folded route, index %d", n, index);
}

int dpb_engine_stats(const dpb_engine* e, int64_t* launches, double* gemm_flops, double* gemm_bytes) {
  if (!e) return fail("null engine");
  if (launches) *launches = e->n_launch;
  if (gemm_flops) *gemm_flops = e->flops;
  if (gemm_bytes) *gemm_bytes = e->gbytes;
  return 0;
}

}  // extern "C"
