// The h-space guidance edit (Kwon et al., "Diffusion models already have a semantic latent space": Asyrp; the reference's edit_ht == 'h_space_guidance',
// src/modules/edit.py:1232-1245, :1500-1513, whose h_space_guidance method it never defines): at every DDIM step of the guided interval the net runs
// twice, plain (e) and with the tap shifted by sigma c (e_s), and the two halves of the DDIM update take their own mix of the two,
//   d = e_s - e,  eP = e + gP d,  eD = e + gD d,  P = (x - eP sqrt(1-a)) / sqrt(a),  x' = sqrt(a') P + sqrt(1-a') eD        (eta = 0)
// (gP, gD) = (1, 0): Asyrp's asymmetric process; (1, 1): the plain DDIM step of the shifted net.  The U-Net passes are the engine's; this file holds
//   the asymmetric DDIM step   (x, e, e_s) -> x', optionally P, and per row (sum d^2, flag) in fp64
// (the grouped tap shift, the seam of dpb_forward_shift_groups, is shift_tap_kernel of elementwise.hip).
// The step is fp32 in the operation order of ddim_kernel (elementwise.hip): d, eP and eD are formed first with one rounding each, so a row with d == 0
// or gP == gD == 0 is dpb_ddim_step on (x, e) bit for bit.  The sum of d^2 follows chain.hip: thread t of a workgroup adds the elements of its groups of
// four in index order in fp64, the 256 accumulators meet in block_sum, and a row's slices of ROW_SLICE elements are added in slice order; no atomics, so a
// row's results are a function of the row and N only -- not of n, of the row's position in the stack or of the alignment of its pointers.
#include "kernels.h"
#include "geom.h"

namespace dpb {

namespace {

constexpr long HG_MAX_ROWS = 32768;         // rows per launch (gridDim.y)

__device__ inline bool hg_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }   // false for NaN and +-inf

// part[b][slice] = (sum d^2 of the slice in fp64, number of non-finite elements of x, e and e_s in it)
__global__ __launch_bounds__(ROW_NT) void hguide_partial_kernel(const float* x, const float* e, const float* es, long N, double* part) {
  __shared__ double red[ROW_NT / 64];
  const int b = blockIdx.y, t = threadIdx.x;
  const long nsl = gridDim.x, off = (long)b * N;
  const bool alx = aligned16(x + off), ale = aligned16(e + off), als = aligned16(es + off);
  double s2 = 0.0, bad = 0.0;
#pragma unroll
  for (int i = 0; i < ROW_GROUPS; ++i) {
    const long j = (long)blockIdx.x * ROW_SLICE + ((long)i * ROW_NT + t) * 4;
    if (j < N) {
      const float4 xv = row_load4(x + off, j, N, alx), ev = row_load4(e + off, j, N, ale), sv = row_load4(es + off, j, N, als);
      const float xi[4] = {xv.x, xv.y, xv.z, xv.w}, ei[4] = {ev.x, ev.y, ev.z, ev.w}, si[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double d = (double)(si[c] - ei[c]);          // the fp32 difference the step uses, widened
        s2 += d * d;
        if (!hg_finite(xi[c]) || !hg_finite(ei[c]) || !hg_finite(si[c])) bad += 1.0;
      }
    }
  }
  s2 = block_sum<ROW_NT>(s2, red);
  bad = block_sum<ROW_NT>(bad, red);
  if (t == 0) {
    double* p = part + ((long)b * nsl + blockIdx.x) * 2;
    p[0] = s2; p[1] = bad;
  }
}

// One element of the step.  The order and the fused operations are those the compiler gives ddim_kernel -- p = (x - e s1a) / sa with the product fused into
// the subtraction, out = san p + s1an e as two rounded products and their sum -- written out so that they do not depend on it here.
struct HgCoef { float sa, s1a, san, s1an, gP, gD; };
__device__ inline void hg_elem(float x, float e, float es, const HgCoef& k, float& p, float& o) {
#pragma clang fp contract(off)
  const float d = es - e;
  const float eP = __builtin_fmaf(k.gP, d, e), eD = __builtin_fmaf(k.gD, d, e);
  p = __builtin_fmaf(-eP, k.s1a, x) / k.sa;
  o = k.san * p + k.s1an * eD;
}

// out = the step, x0 = P (optional); the workgroup of slice 0 writes the row's (sum d^2, flag); a flagged row is NaN in out and x0
__global__ __launch_bounds__(ROW_NT) void hguide_apply_kernel(const float* x, const float* e, const float* es, float* out, float* x0, long N, HgCoef k,
                                                             const double* part, double* stats) {
  __shared__ double row_s[2];
  const int b = blockIdx.y, t = threadIdx.x;
  const long nsl = gridDim.x, off = (long)b * N;
  if (t == 0) sum_slices<2>(part + (long)b * nsl * 2, nsl, row_s);
  __syncthreads();
  const bool bad = row_s[1] != 0.0;
  const float nanf_ = __builtin_nanf("");
  const bool alx = aligned16(x + off), ale = aligned16(e + off), als = aligned16(es + off), alo = aligned16(out + off),
             alp = x0 && aligned16(x0 + off);
#pragma unroll
  for (int i = 0; i < ROW_GROUPS; ++i) {
    const long j = (long)blockIdx.x * ROW_SLICE + ((long)i * ROW_NT + t) * 4;
    if (j >= N) continue;
    const float4 xv = row_load4(x + off, j, N, alx), ev = row_load4(e + off, j, N, ale), sv = row_load4(es + off, j, N, als);
    const float xi[4] = {xv.x, xv.y, xv.z, xv.w}, ei[4] = {ev.x, ev.y, ev.z, ev.w}, si[4] = {sv.x, sv.y, sv.z, sv.w};
    float po[4], oo[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      hg_elem(xi[c], ei[c], si[c], k, po[c], oo[c]);
      if (bad) { po[c] = nanf_; oo[c] = nanf_; }
    }
    row_store4(out + off, j, N, alo, make_float4(oo[0], oo[1], oo[2], oo[3]));
    if (x0) row_store4(x0 + off, j, N, alp, make_float4(po[0], po[1], po[2], po[3]));
  }
  if (t == 0 && blockIdx.x == 0) { stats[(long)b * 2] = row_s[0]; stats[(long)b * 2 + 1] = bad ? 1.0 : 0.0; }
}

}  // namespace

size_t ddim_step_asym_scratch_bytes(long n, long N) { return row_partial_bytes(n, N); }

int launch_ddim_step_asym(const float* x, const float* e, const float* es, float* out, float* x0, long n, long N, float a_t, float a_next, float gP,
                          float gD, double* stats, void* scratch, size_t scratch_bytes, hipStream_t st) {
  if (check_rows("ddim_step_asym", n, N)) return -1;
  const long nsl = row_slices(N);
  if (!std::isfinite(a_t) || !std::isfinite(a_next) || !std::isfinite(gP) || !std::isfinite(gD)) {
    set_error("ddim_step_asym: a non-finite scalar (alpha_t=%g, alpha_next=%g, gP=%g, gD=%g)", a_t, a_next, gP, gD);
    return -1;
  }
  if (!(a_t > 0.f && a_t <= 1.f) || !(a_next > 0.f && a_next <= 1.f)) {
    set_error("ddim_step_asym: alpha_t=%g and alpha_next=%g must lie in (0, 1]", a_t, a_next);
    return -1;
  }
  if (scratch_bytes < ddim_step_asym_scratch_bytes(n, N)) {
    set_error("ddim_step_asym: scratch of %zu bytes, dpb_ddim_step_asym_scratch_bytes(%ld, %ld) = %zu", scratch_bytes, n, N, ddim_step_asym_scratch_bytes(n, N));
    return -1;
  }
  if ((uintptr_t)scratch & 7 || (uintptr_t)stats & 7) { set_error("ddim_step_asym: scratch and stats must be 8-byte aligned"); return -1; }
  // the square roots in fp32 of the fp32 alphas, as launch_ddim_step (utils.py:301-306)
  const HgCoef k{sqrtf(a_t), sqrtf(1.f - a_t), sqrtf(a_next), sqrtf(1.f - a_next), gP, gD};
  double* part = (double*)scratch;
  for (long r0 = 0; r0 < n; r0 += HG_MAX_ROWS) {
    const long rows = std::min(HG_MAX_ROWS, n - r0), o = r0 * N;
    const dim3 grid((unsigned)nsl, (unsigned)rows), block(ROW_NT);
    DPB_LAUNCH(hguide_partial_kernel, grid, block, 0, st, x + o, e + o, es + o, N, part + r0 * nsl * 2);
    DPB_LAUNCH(hguide_apply_kernel, grid, block, 0, st, x + o, e + o, es + o, out + o, x0 ? x0 + o : nullptr, N, k, (const double*)(part + r0 * nsl * 2),
               stats + r0 * 2);
  }
  DPB_CHECK(hipGetLastError());
  return 0;
}

}  // namespace dpb
