// CGLS between the U-Net passes: min_d ||J d - c||^2 + mu ||d||^2 from d = 0, for R independent rows at once (include/dpb.h "The least-squares
// inverse").  The tangent and adjoint passes are the engine's (q = J p, w = J^T r); this file holds the recurrence between them:
//   init     d = 0, r = c, p = s = w0 (= J^T c, supplied), gamma = gamma0 = ||s||^2, mu = mu_abs + mu_rel gamma0 / ||c||^2
//   h-step   alpha = gamma / (||q||^2 + mu ||p||^2), d <- d + alpha p, r <- r - alpha q
//   x-step   s = w - mu d, gamma' = ||s||^2, beta = gamma' / gamma, p <- s + beta p, gamma <- gamma'
// and the two kernels of the newton-h chain around an inner solve: the residual res = h0 + f sigma c - h and the clamped update x + kappa d.
// The scheme is chain.hip's: a partial kernel leaves one fp64 sum per slice of ROW_SLICE elements, an apply kernel adds a row's slices in slice order
// (sum_slices: the same chain in every workgroup of the row) and forms the new elements in fp64 from fp32 operands, rounded once; a third kernel of one
// thread per row writes the row's scalars, so that no workgroup reads a scalar another one of the same launch writes.  No floating-point atomics: a
// row's bits are a function of that row, N and D only -- not of R, of the row's place in the stack or of the alignment of its pointers (the 16-byte
// and the 4-byte paths give every thread the same elements in the same order).  A launch takes at most CHAIN_MAX_ROWS rows: rows are a grid axis.
//
// A launch covers the N-side vectors (d, p, w: slices 0 .. nslN-1 of the grid) and the D-side vectors (r, q, c: the nslD slices after them).
// state [R][8] fp64: gamma, gamma0, mu, ||r||^2, ||d||^2, flag, ||c||^2, x-steps taken.  A row whose flag is not 0 is frozen: the kernels neither read
// its inputs nor write its vectors, so d, r and p pass through every later step bit for bit.
#include "kernels.h"
#include "geom.h"

namespace dpb {

namespace {

enum { ST_GAMMA = 0, ST_GAMMA0, ST_MU, ST_RR, ST_DD, ST_FLAG, ST_CC, ST_ITERS };

__device__ inline bool finite64(double v) { return fabs(v) < 1.7976931348623157e308; }      // false for NaN and inf

// the sum of squares of this workgroup's slice of a row (thread t: its ROW_GROUPS groups of four in index order), the same value in every thread
__device__ inline double slice_sumsq(const float* row, long sl, long n, double* red) {
  const bool al = aligned16(row);
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < ROW_GROUPS; ++i) {
    const long j = sl * ROW_SLICE + ((long)i * ROW_NT + threadIdx.x) * 4;
    if (j < n) {
      const float4 v = row_load4(row, j, n, al);
      const double a0 = v.x, a1 = v.y, a2 = v.z, a3 = v.w;
      s += a0 * a0; s += a1 * a1; s += a2 * a2; s += a3 * a3;
    }
  }
  return block_sum<ROW_NT>(s, red);
}

// this workgroup's slice of row <- v
__device__ inline void slice_fill(float* row, long sl, long n, float v) {
  const bool al = aligned16(row);
#pragma unroll
  for (int i = 0; i < ROW_GROUPS; ++i) {
    const long j = sl * ROW_SLICE + ((long)i * ROW_NT + threadIdx.x) * 4;
    if (j < n) row_store4(row, j, n, al, make_float4(v, v, v, v));
  }
}

// out = fl32(a + f b) on this workgroup's slice (out may be a); returns the slice's sum of out^2.  b2: with it, b is (b - g b2) formed in fp64 first
__device__ inline double slice_axpy(const float* a, double f, const float* b, double g, const float* b2, float* out, long sl, long n, double* red) {
  const bool ala = aligned16(a), alb = aligned16(b), alc = b2 && aligned16(b2), alo = aligned16(out);
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < ROW_GROUPS; ++i) {
    const long j = sl * ROW_SLICE + ((long)i * ROW_NT + threadIdx.x) * 4;
    if (j >= n) continue;
    const float4 av = row_load4(a, j, n, ala), bv = row_load4(b, j, n, alb);
    const float4 cv = b2 ? row_load4(b2, j, n, alc) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float ai[4] = {av.x, av.y, av.z, av.w}, bi[4] = {bv.x, bv.y, bv.z, bv.w}, ci[4] = {cv.x, cv.y, cv.z, cv.w};
    float o[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const double bb = b2 ? (double)bi[c] - g * (double)ci[c] : (double)bi[c];
      // a + f b with a as the SCALED operand when b2 is given (p <- s + beta p: a = p, f = beta, b = w, b2 = d)
      o[c] = b2 ? (float)(bb + f * (double)ai[c]) : (float)((double)ai[c] + f * bb);
      if (j + c < n) s += (double)o[c] * (double)o[c];
    }
    row_store4(out, j, n, alo, make_float4(o[0], o[1], o[2], o[3]));
  }
  return block_sum<ROW_NT>(s, red);
}

// ---- init
// part1[b][slice]: slices < nslN sum w0^2, the others sum c^2
__global__ __launch_bounds__(ROW_NT) void cgls_init_partial_kernel(const float* c, const float* w0, long N, long D, long nslN, double* part1) {
  __shared__ double red[ROW_NT / 64];
  const long b = blockIdx.y, sl = blockIdx.x, nsl = gridDim.x;
  const double s = sl < nslN ? slice_sumsq(w0 + b * N, sl, N, red) : slice_sumsq(c + b * D, sl - nslN, D, red);
  if (threadIdx.x == 0) part1[b * nsl + sl] = s;
}

// the scalars of a row at init from its two sums; returns the flag
__device__ inline int init_scalars(double g0, double cc, double mu_abs, double mu_rel, double tol, double* mu) {
  *mu = mu_abs;
  if (!finite64(g0) || !finite64(cc)) return 3;
  if (g0 <= tol * tol * g0) return 1;                          // (gamma0 = 0 included)
  if (!(cc > 0.0)) return 2;                                   // J^T c != 0 with c = 0: the supplied w0 is not J^T c; mu_rel has no scale
  *mu = mu_abs + mu_rel * g0 / cc;
  return finite64(*mu) ? 0 : 2;
}

__global__ __launch_bounds__(ROW_NT) void cgls_init_apply_kernel(const float* c, const float* w0, float* delta, float* r, float* p, long N, long D,
                                                                long nslN, double mu_abs, double mu_rel, double tol, const double* part1) {
  __shared__ double tot[2];
  const long b = blockIdx.y, sl = blockIdx.x, nsl = gridDim.x;
  if (threadIdx.x == 0) {
    sum_slices<1>(part1 + b * nsl, nslN, tot);
    sum_slices<1>(part1 + b * nsl + nslN, nsl - nslN, tot + 1);
  }
  __syncthreads();
  double mu;
  const bool bad = init_scalars(tot[0], tot[1], mu_abs, mu_rel, tol, &mu) == 3;
  const float nanf_ = __builtin_nanf("");
  if (sl < nslN) {
    slice_fill(delta + b * N, sl, N, bad ? nanf_ : 0.f);
    const float *src = w0 + b * N; float* dst = p + b * N;
    const bool als = aligned16(src), ald = aligned16(dst);
#pragma unroll
    for (int i = 0; i < ROW_GROUPS; ++i) {
      const long j = sl * ROW_SLICE + ((long)i * ROW_NT + threadIdx.x) * 4;
      if (j < N) row_store4(dst, j, N, ald, bad ? make_float4(nanf_, nanf_, nanf_, nanf_) : row_load4(src, j, N, als));
    }
  } else {
    const float *src = c + b * D; float* dst = r + b * D;
    const bool als = aligned16(src), ald = aligned16(dst);
#pragma unroll
    for (int i = 0; i < ROW_GROUPS; ++i) {
      const long j = (sl - nslN) * ROW_SLICE + ((long)i * ROW_NT + threadIdx.x) * 4;
      if (j < D) row_store4(dst, j, D, ald, bad ? make_float4(nanf_, nanf_, nanf_, nanf_) : row_load4(src, j, D, als));
    }
  }
}

__device__ inline void write_hist(double* hist, const double* st) {
  hist[0] = st[ST_GAMMA]; hist[1] = st[ST_RR]; hist[2] = st[ST_DD]; hist[3] = st[ST_FLAG];
}

// one thread per row
__global__ __launch_bounds__(ROW_NT) void cgls_init_final_kernel(long rows, long nslN, long nsl, double mu_abs, double mu_rel, double tol,
                                                                const double* part1, double* state, double* hist) {
  const long b = (long)blockIdx.x * ROW_NT + threadIdx.x;
  if (b >= rows) return;
  double g0, cc, mu;
  sum_slices<1>(part1 + b * nsl, nslN, &g0);
  sum_slices<1>(part1 + b * nsl + nslN, nsl - nslN, &cc);
  const int flag = init_scalars(g0, cc, mu_abs, mu_rel, tol, &mu);
  double* st = state + b * 8;
  const double nan = nan64();
  st[ST_GAMMA] = flag == 3 ? nan : g0; st[ST_GAMMA0] = flag == 3 ? nan : g0; st[ST_MU] = flag == 3 ? nan : mu;
  st[ST_RR] = flag == 3 ? nan : cc; st[ST_DD] = flag == 3 ? nan : 0.0; st[ST_FLAG] = (double)flag; st[ST_CC] = flag == 3 ? nan : cc; st[ST_ITERS] = 0.0;
  write_hist(hist + b * 4, st);
}

// ---- h-step
// part1[b][slice]: slices < nslN sum p^2, the others sum q^2; a frozen row's inputs are not read
__global__ __launch_bounds__(ROW_NT) void cgls_h_partial_kernel(const float* q, const float* p, long N, long D, long nslN, const double* state,
                                                               double* part1) {
  __shared__ double red[ROW_NT / 64];
  const long b = blockIdx.y, sl = blockIdx.x, nsl = gridDim.x;
  if (state[b * 8 + ST_FLAG] != 0.0) return;
  const double s = sl < nslN ? slice_sumsq(p + b * N, sl, N, red) : slice_sumsq(q + b * D, sl - nslN, D, red);
  if (threadIdx.x == 0) part1[b * nsl + sl] = s;
}

// alpha of a live row from its two sums; returns the flag the step raises (0, 2 or 3)
__device__ inline int h_scalars(double pp, double qq, double gamma, double mu, double* alpha) {
  *alpha = 0.0;
  if (!finite64(pp) || !finite64(qq)) return 3;
  const double den = qq + mu * pp;
  if (!(den > 0.0) || !finite64(den)) return 2;
  *alpha = gamma / den;
  return 0;
}

// d <- fl32(d + alpha p), r <- fl32(r - alpha q); part2[b][slice] = the sums of squares of the new slices
__global__ __launch_bounds__(ROW_NT) void cgls_h_apply_kernel(const float* q, float* delta, float* r, float* p, long N, long D, long nslN,
                                                             const double* state, const double* part1, double* part2) {
  __shared__ double red[ROW_NT / 64];
  __shared__ double tot[2];
  const long b = blockIdx.y, sl = blockIdx.x, nsl = gridDim.x;
  const double* st = state + b * 8;
  if (st[ST_FLAG] != 0.0) return;
  if (threadIdx.x == 0) {
    sum_slices<1>(part1 + b * nsl, nslN, tot);
    sum_slices<1>(part1 + b * nsl + nslN, nsl - nslN, tot + 1);
  }
  __syncthreads();
  double alpha;
  const int flag = h_scalars(tot[0], tot[1], st[ST_GAMMA], st[ST_MU], &alpha);
  if (flag == 2) return;
  const float nanf_ = __builtin_nanf("");
  if (flag == 3) {
    if (sl < nslN) { slice_fill(delta + b * N, sl, N, nanf_); slice_fill(p + b * N, sl, N, nanf_); }
    else slice_fill(r + b * D, sl - nslN, D, nanf_);
    return;
  }
  const double s = sl < nslN ? slice_axpy(delta + b * N, alpha, p + b * N, 0.0, nullptr, delta + b * N, sl, N, red)
                             : slice_axpy(r + b * D, -alpha, q + b * D, 0.0, nullptr, r + b * D, sl - nslN, D, red);
  if (threadIdx.x == 0) part2[b * nsl + sl] = s;
}

__global__ __launch_bounds__(ROW_NT) void cgls_h_final_kernel(long rows, long nslN, long nsl, const double* part1, const double* part2, double* state,
                                                             double* hist) {
  const long b = (long)blockIdx.x * ROW_NT + threadIdx.x;
  if (b >= rows) return;
  double* st = state + b * 8;
  if (st[ST_FLAG] == 0.0) {
    double pp, qq, alpha;
    sum_slices<1>(part1 + b * nsl, nslN, &pp);
    sum_slices<1>(part1 + b * nsl + nslN, nsl - nslN, &qq);
    const int flag = h_scalars(pp, qq, st[ST_GAMMA], st[ST_MU], &alpha);
    if (flag == 3) {
      const double nan = nan64();
      st[ST_GAMMA] = nan; st[ST_RR] = nan; st[ST_DD] = nan;
    } else if (flag == 0) {
      sum_slices<1>(part2 + b * nsl, nslN, st + ST_DD);
      sum_slices<1>(part2 + b * nsl + nslN, nsl - nslN, st + ST_RR);
    }
    st[ST_FLAG] = (double)flag;
  }
  write_hist(hist + b * 4, st);
}

// ---- x-step
// part1[b][slice < nslN] = the slice's sum of s^2, s = w - mu d in fp64
__global__ __launch_bounds__(ROW_NT) void cgls_x_partial_kernel(const float* w, const float* delta, long N, const double* state, double* part1) {
  __shared__ double red[ROW_NT / 64];
  const long b = blockIdx.y, sl = blockIdx.x, nsl = gridDim.x;
  const double* st = state + b * 8;
  if (st[ST_FLAG] != 0.0) return;
  const double mu = st[ST_MU];
  const float *wr = w + b * N, *dr = delta + b * N;
  const bool alw = aligned16(wr), ald = aligned16(dr);
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < ROW_GROUPS; ++i) {
    const long j = sl * ROW_SLICE + ((long)i * ROW_NT + threadIdx.x) * 4;
    if (j < N) {
      const float4 wv = row_load4(wr, j, N, alw), dv = row_load4(dr, j, N, ald);
      const double s0 = (double)wv.x - mu * (double)dv.x, s1 = (double)wv.y - mu * (double)dv.y;
      const double s2 = (double)wv.z - mu * (double)dv.z, s3 = (double)wv.w - mu * (double)dv.w;
      s += s0 * s0; s += s1 * s1; s += s2 * s2; s += s3 * s3;
    }
  }
  s = block_sum<ROW_NT>(s, red);
  if (threadIdx.x == 0) part1[b * nsl + sl] = s;
}

// p <- fl32((w - mu d) + beta p); a non-finite w: NaN into d, p and (the D-side workgroups) r
__global__ __launch_bounds__(ROW_NT) void cgls_x_apply_kernel(const float* w, float* delta, float* r, float* p, long N, long D, long nslN,
                                                             const double* state, const double* part1) {
  __shared__ double red[ROW_NT / 64];
  __shared__ double tot[1];
  const long b = blockIdx.y, sl = blockIdx.x;
  const double* st = state + b * 8;
  if (st[ST_FLAG] != 0.0) return;
  if (threadIdx.x == 0) sum_slices<1>(part1 + b * nslN, nslN, tot);
  __syncthreads();
  const double g1 = tot[0];
  const float nanf_ = __builtin_nanf("");
  if (!finite64(g1)) {
    if (sl < nslN) { slice_fill(delta + b * N, sl, N, nanf_); slice_fill(p + b * N, sl, N, nanf_); }
    else slice_fill(r + b * D, sl - nslN, D, nanf_);
    return;
  }
  if (sl >= nslN) return;
  const double beta = g1 / st[ST_GAMMA];                        // a live row has gamma > tol^2 gamma0 >= 0
  (void)slice_axpy(p + b * N, beta, w + b * N, st[ST_MU], delta + b * N, p + b * N, sl, N, red);
}

__global__ __launch_bounds__(ROW_NT) void cgls_x_final_kernel(long rows, long nslN, double tol, const double* part1, double* state, double* hist) {
  const long b = (long)blockIdx.x * ROW_NT + threadIdx.x;
  if (b >= rows) return;
  double* st = state + b * 8;
  if (st[ST_FLAG] == 0.0) {
    double g1;
    sum_slices<1>(part1 + b * nslN, nslN, &g1);
    st[ST_ITERS] += 1.0;
    if (!finite64(g1)) {
      const double nan = nan64();
      st[ST_GAMMA] = nan; st[ST_RR] = nan; st[ST_DD] = nan; st[ST_FLAG] = 3.0;
    } else {
      st[ST_GAMMA] = g1;
      if (g1 <= tol * tol * st[ST_GAMMA0]) st[ST_FLAG] = 1.0;
    }
  }
  write_hist(hist + b * 4, st);
}

// ---- the newton-h chain
struct NewtonDirs { int dir[CHAIN_MAX_ROWS]; float sign[CHAIN_MAX_ROWS]; float scale[CHAIN_MAX_ROWS]; };

// res[b][j] = fl32(h0 + (frac scale[b]) (sign[b] u[dir[b]]) - h), formed in fp64
__global__ __launch_bounds__(ROW_NT) void newton_residual_kernel(const float* h0, const float* h, const float* u, long D, NewtonDirs dirs, double frac,
                                                                float* res) {
  const long b = blockIdx.y;
  const long j = ((long)blockIdx.x * ROW_NT + threadIdx.x) * 4;
  if (j >= D) return;
  const float *gr = h0 + b * D, *hr = h + b * D, *ur = u + (long)dirs.dir[b] * D;
  float* rr = res + b * D;
  const float4 g = row_load4(gr, j, D, aligned16(gr)), a = row_load4(hr, j, D, aligned16(hr)), c = row_load4(ur, j, D, aligned16(ur));
  const double f = frac * (double)dirs.scale[b], sg = (double)dirs.sign[b];
  float4 o;
  o.x = (float)(((double)g.x + f * (sg * (double)c.x)) - (double)a.x);
  o.y = (float)(((double)g.y + f * (sg * (double)c.y)) - (double)a.y);
  o.z = (float)(((double)g.z + f * (sg * (double)c.z)) - (double)a.z);
  o.w = (float)(((double)g.w + f * (sg * (double)c.w)) - (double)a.w);
  row_store4(rr, j, D, aligned16(rr), o);
}

// x_out = fl32(x + kappa d), kappa = min(1, radius / ||d||) (radius = 0: 1), ||d||^2 from the solver's state; the workgroup of slice 0 writes
// step_stats[b] = (||res||^2, ||d||^2, kappa, flag)
__global__ __launch_bounds__(ROW_NT) void newton_update_kernel(const float* x, const float* delta, const double* state, double radius, float* x_out,
                                                              double* step_stats, long N) {
  const long b = blockIdx.y, sl = blockIdx.x;
  const double* st = state + b * 8;
  const double dd = st[ST_DD];
  double kappa = 1.0;
  if (radius > 0.0 && dd > radius * radius) kappa = radius / sqrt(dd);
  const float *xr = x + b * N, *dr = delta + b * N;
  float* orow = x_out + b * N;
  const bool alx = aligned16(xr), ald = aligned16(dr), alo = aligned16(orow);
#pragma unroll
  for (int i = 0; i < ROW_GROUPS; ++i) {
    const long j = sl * ROW_SLICE + ((long)i * ROW_NT + threadIdx.x) * 4;
    if (j >= N) continue;
    const float4 xv = row_load4(xr, j, N, alx), dv = row_load4(dr, j, N, ald);
    float4 o;
    o.x = (float)((double)xv.x + kappa * (double)dv.x);
    o.y = (float)((double)xv.y + kappa * (double)dv.y);
    o.z = (float)((double)xv.z + kappa * (double)dv.z);
    o.w = (float)((double)xv.w + kappa * (double)dv.w);
    row_store4(orow, j, N, alo, o);
  }
  if (sl == 0 && threadIdx.x == 0) {
    double* o = step_stats + b * 4;
    o[0] = st[ST_CC]; o[1] = dd; o[2] = dd == dd ? kappa : nan64(); o[3] = st[ST_FLAG];
  }
}

// the shape, the scratch and the pointers of a solver call
int check_cgls(const char* who, long R, long N, long D, const void* state, const void* hist, const void* scratch, size_t scratch_bytes) {
  if (R < 1 || R > 0x7fffffffL) { set_error("%s: R=%ld rows outside [1, 2^31)", who, R); return -1; }
  if (N < 1) { set_error("%s: N=%ld < 1", who, N); return -1; }
  if (D < 1) { set_error("%s: D=%ld < 1", who, D); return -1; }
  if (row_slices(N) + row_slices(D) > 0x7fffffffL) { set_error("%s: rows of %ld and %ld elements are too long", who, N, D); return -1; }
  if (scratch_bytes < cgls_scratch_bytes(R, N, D)) {
    set_error("%s: scratch of %zu bytes, %s_scratch_bytes(%ld, %ld, %ld) = %zu", who, scratch_bytes, who, R, N, D, cgls_scratch_bytes(R, N, D));
    return -1;
  }
  if ((uintptr_t)scratch & 7 || (uintptr_t)state & 7 || (uintptr_t)hist & 7) { set_error("%s: scratch, state and hist must be 8-byte aligned", who); return -1; }
  return 0;
}

int check_scalar(const char* who, const char* name, double v) {
  if (!(v >= 0.0) || !std::isfinite(v)) { set_error("%s: %s=%g must be finite and not negative", who, name, v); return -1; }
  return 0;
}

}  // namespace

// two sets of per-slice sums (before and after the update), one fp64 value per slice of the N side and of the D side
size_t cgls_scratch_bytes(long R, long N, long D) {
  if (R < 1 || N < 1 || D < 1) return 0;
  return (size_t)R * (size_t)(row_slices(N) + row_slices(D)) * 2 * sizeof(double);
}

int launch_cgls_init(const float* c, const float* w0, float* delta, float* r, float* p, double* state, double* hist, double mu_abs, double mu_rel,
                     double tol, long R, long N, long D, void* scratch, size_t scratch_bytes, hipStream_t st) {
  if (check_cgls("dpb_cgls_init", R, N, D, state, hist, scratch, scratch_bytes)) return -1;
  if (check_scalar("dpb_cgls_init", "mu_abs", mu_abs) || check_scalar("dpb_cgls_init", "mu_rel", mu_rel) || check_scalar("dpb_cgls_init", "tol", tol))
    return -1;
  const long nslN = row_slices(N), nsl = nslN + row_slices(D);
  double* part1 = (double*)scratch;
  for (long r0 = 0; r0 < R; r0 += CHAIN_MAX_ROWS) {
    const long rows = std::min<long>(CHAIN_MAX_ROWS, R - r0);
    const dim3 grid((unsigned)nsl, (unsigned)rows), block(ROW_NT);
    double* p1 = part1 + r0 * nsl;
    DPB_LAUNCH(cgls_init_partial_kernel, grid, block, 0, st, c + r0 * D, w0 + r0 * N, N, D, nslN, p1);
    DPB_LAUNCH(cgls_init_apply_kernel, grid, block, 0, st, c + r0 * D, w0 + r0 * N, delta + r0 * N, r + r0 * D, p + r0 * N, N, D, nslN, mu_abs, mu_rel,
               tol, (const double*)p1);
    DPB_LAUNCH(cgls_init_final_kernel, dim3(1), block, 0, st, rows, nslN, nsl, mu_abs, mu_rel, tol, (const double*)p1, state + r0 * 8, hist + r0 * 4);
  }
  DPB_CHECK(hipGetLastError());
  return 0;
}

int launch_cgls_h_step(const float* q, float* delta, float* r, float* p, double* state, double* hist, long R, long N, long D, void* scratch,
                       size_t scratch_bytes, hipStream_t st) {
  if (check_cgls("dpb_cgls_h_step", R, N, D, state, hist, scratch, scratch_bytes)) return -1;
  const long nslN = row_slices(N), nsl = nslN + row_slices(D);
  double *part1 = (double*)scratch, *part2 = part1 + R * nsl;
  for (long r0 = 0; r0 < R; r0 += CHAIN_MAX_ROWS) {
    const long rows = std::min<long>(CHAIN_MAX_ROWS, R - r0);
    const dim3 grid((unsigned)nsl, (unsigned)rows), block(ROW_NT);
    double *p1 = part1 + r0 * nsl, *p2 = part2 + r0 * nsl, *s = state + r0 * 8;
    DPB_LAUNCH(cgls_h_partial_kernel, grid, block, 0, st, q + r0 * D, (const float*)(p + r0 * N), N, D, nslN, (const double*)s, p1);
    DPB_LAUNCH(cgls_h_apply_kernel, grid, block, 0, st, q + r0 * D, delta + r0 * N, r + r0 * D, p + r0 * N, N, D, nslN, (const double*)s,
               (const double*)p1, p2);
    DPB_LAUNCH(cgls_h_final_kernel, dim3(1), block, 0, st, rows, nslN, nsl, (const double*)p1, (const double*)p2, s, hist + r0 * 4);
  }
  DPB_CHECK(hipGetLastError());
  return 0;
}

int launch_cgls_x_step(const float* w, float* delta, float* r, float* p, double* state, double* hist, double tol, long R, long N, long D, void* scratch,
                       size_t scratch_bytes, hipStream_t st) {
  if (check_cgls("dpb_cgls_x_step", R, N, D, state, hist, scratch, scratch_bytes)) return -1;
  if (check_scalar("dpb_cgls_x_step", "tol", tol)) return -1;
  const long nslN = row_slices(N), nsl = nslN + row_slices(D);
  double* part1 = (double*)scratch;
  for (long r0 = 0; r0 < R; r0 += CHAIN_MAX_ROWS) {
    const long rows = std::min<long>(CHAIN_MAX_ROWS, R - r0);
    const dim3 block(ROW_NT);
    double *p1 = part1 + r0 * nslN, *s = state + r0 * 8;
    DPB_LAUNCH(cgls_x_partial_kernel, dim3((unsigned)nslN, (unsigned)rows), block, 0, st, w + r0 * N, (const float*)(delta + r0 * N), N,
               (const double*)s, p1);
    DPB_LAUNCH(cgls_x_apply_kernel, dim3((unsigned)nsl, (unsigned)rows), block, 0, st, w + r0 * N, delta + r0 * N, r + r0 * D, p + r0 * N, N, D, nslN,
               (const double*)s, (const double*)p1);
    DPB_LAUNCH(cgls_x_final_kernel, dim3(1), block, 0, st, rows, nslN, tol, (const double*)p1, s, hist + r0 * 4);
  }
  DPB_CHECK(hipGetLastError());
  return 0;
}

int launch_newton_residual(const float* h0, const float* h, const float* u, int nu, const int32_t* dir, const float* sign, const float* scale,
                           double frac, long n, long D, float* res, hipStream_t st) {
  if (check_rows("newton_residual", n, D)) return -1;
  if (nu < 1) { set_error("newton_residual: nu=%d: at least one direction is needed", nu); return -1; }
  if (!std::isfinite(frac)) { set_error("newton_residual: frac is not finite"); return -1; }
  const long ng = (D + 3) / 4;
  for (long r0 = 0; r0 < n; r0 += CHAIN_MAX_ROWS) {
    const int rows = (int)std::min<long>(CHAIN_MAX_ROWS, n - r0);
    NewtonDirs d;
    for (int i = 0; i < rows; ++i) {
      if (dir[r0 + i] < 0 || dir[r0 + i] >= nu) { set_error("newton_residual: dir[%ld]=%d outside [0,%d)", r0 + i, dir[r0 + i], nu); return -1; }
      if (!std::isfinite(sign[r0 + i])) { set_error("newton_residual: sign[%ld] is not finite", r0 + i); return -1; }
      if (!std::isfinite(scale[r0 + i])) { set_error("newton_residual: scale[%ld] is not finite", r0 + i); return -1; }
      d.dir[i] = dir[r0 + i]; d.sign[i] = sign[r0 + i]; d.scale[i] = scale[r0 + i];
    }
    DPB_LAUNCH(newton_residual_kernel, dim3((unsigned)((ng + ROW_NT - 1) / ROW_NT), (unsigned)rows), dim3(ROW_NT), 0, st, h0 + r0 * D, h + r0 * D, u, D,
               d, frac, res + r0 * D);
  }
  DPB_CHECK(hipGetLastError());
  return 0;
}

int launch_newton_update(const float* x, const float* delta, const double* state, double radius, float* x_out, double* step_stats, long n, long N,
                         hipStream_t st) {
  if (check_rows("newton_update", n, N)) return -1;
  if (!(radius >= 0.0) || !std::isfinite(radius)) { set_error("newton_update: radius=%g must be finite and not negative (0: no clamp)", radius); return -1; }
  if ((uintptr_t)state & 7 || (uintptr_t)step_stats & 7) { set_error("newton_update: state and step_stats must be 8-byte aligned"); return -1; }
  const long nsl = row_slices(N);
  for (long r0 = 0; r0 < n; r0 += CHAIN_MAX_ROWS) {
    const long rows = std::min<long>(CHAIN_MAX_ROWS, n - r0);
    DPB_LAUNCH(newton_update_kernel, dim3((unsigned)nsl, (unsigned)rows), dim3(ROW_NT), 0, st, x + r0 * N, delta + r0 * N, state + r0 * 8, radius,
               x_out + r0 * N, step_stats + r0 * 4, N);
  }
  DPB_CHECK(hipGetLastError());
  return 0;
}

}  // namespace dpb
