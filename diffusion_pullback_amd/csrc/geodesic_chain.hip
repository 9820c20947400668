// Pullback geodesics between two latents: a curve P_0 = x_a, P_1 .. P_m, P_{m+1} = x_b at one timestep, h_i = get_h(P_i), and the discrete energy
//   E = 1/2 sum_{i=0..m} ||h_{i+1} - h_i||^2 + 1/2 lambda sum_{i=0..m} ||P_{i+1} - P_i||^2,
// whose gradient at an interior point is g_i = J(P_i)^T c_i + lambda d_i, c_i = 2 h_i - h_{i-1} - h_{i+1}, d_i = 2 P_i - P_{i-1} - P_{i+1}; one iteration
// is the Jacobi step P_i <- P_i - eta g_i, every g_i from the same old curve.  The U-Net passes are the engine's; this file holds what lies between them:
//   cotangents   h [m+2][D] -> cot_i = fl32(c_i) for the adjoint pass, the segment sums seg_i = ||h_{i+1} - h_i||^2 and csq_i = ||cot_i||^2;
//   update       (P, W = J^T c) -> P_out, the row statistics (sum W^2, sum g^2, sum (P_out - P)^2, flag) and xseg_i = ||P_{i+1} - P_i||^2.
// Unlike the rows of chain.hip and hguide.hip these rows are COUPLED: a point reads its two neighbours.  The frame is the same -- fp32 in / fp32 out,
// every sum in fp64 in one fixed chain (thread t of a workgroup adds the elements of its groups of four in index order, the 256 accumulators meet in
// block_sum, a row's slices of ROW_SLICE elements are added in slice order), no atomics -- so what is computed for point i is a function of rows
// i-1 .. i+1 and the row length only: not of m, of the point's position in the curve or of the alignment of its pointers (the 16-byte and the 4-byte
// access paths give every thread the same elements in the same order).
#include "kernels.h"
#include "geom.h"

namespace dpb {

namespace {

constexpr long GEO_MAX_POINTS = 32768;      // points of a curve, m + 2: the rows are a grid axis of one launch

__device__ inline bool geo_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }   // false for NaN and +-inf

// s <- s + v v as a rounded product and a rounded sum: the cotangent and the update kernel give a segment the same bits, and a host restatement too
__device__ inline void geo_add_sq(double& s, double v) {
#pragma clang fp contract(off)
  const double q = v * v;
  s = s + q;
}

// workgroup (slice, i), i = 0 .. m: the slice's part of segment i (rows i, i+1) and, for i >= 1, cot_i (row i - 1 of cot) and its sum of squares.
// part[i][slice] = (sum (h_{i+1} - h_i)^2, sum cot_i^2).  cot == null (the x-segments of a chain's last curve): the segment sums alone.
__global__ __launch_bounds__(ROW_NT) void geodesic_cot_kernel(const float* h, long D, float* cot, double* part) {
  __shared__ double red[ROW_NT / 64];
  const int i = blockIdx.y, t = threadIdx.x;
  const long nsl = gridDim.x;
  const float *hc = h + (long)i * D, *hn = hc + D, *hp = i > 0 ? hc - D : hc;
  float* cr = i > 0 && cot ? cot + (long)(i - 1) * D : nullptr;
  const bool alc = aligned16(hc), aln = aligned16(hn), alp = aligned16(hp), alo = cr && aligned16(cr);
  double sg = 0.0, sc = 0.0;
#pragma unroll
  for (int g = 0; g < ROW_GROUPS; ++g) {
    const long j = (long)blockIdx.x * ROW_SLICE + ((long)g * ROW_NT + t) * 4;
    if (j >= D) continue;
    const float4 c4 = row_load4(hc, j, D, alc), n4 = row_load4(hn, j, D, aln);
    const float ci[4] = {c4.x, c4.y, c4.z, c4.w}, ni[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
    for (int c = 0; c < 4; ++c)
      geo_add_sq(sg, (double)ni[c] - (double)ci[c]);
    if (cr) {
      const float4 p4 = row_load4(hp, j, D, alp);
      const float pi[4] = {p4.x, p4.y, p4.z, p4.w};
      float o[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        o[c] = (float)((2.0 * (double)ci[c] - (double)pi[c]) - (double)ni[c]);      // (zero past the row's end: the loads are)
        geo_add_sq(sc, (double)o[c]);
      }
      row_store4(cr, j, D, alo, make_float4(o[0], o[1], o[2], o[3]));
    }
  }
  sg = block_sum<ROW_NT>(sg, red);
  sc = block_sum<ROW_NT>(sc, red);
  if (t == 0) {
    double* p = part + ((long)i * nsl + blockIdx.x) * 2;
    p[0] = sg; p[1] = sc;
  }
}

// seg[i] and csq[i - 1] (optional): the slices of part row i in index order; one thread per segment
__global__ void geodesic_cot_finish_kernel(const double* part, long nsl, int nseg, double* seg, double* csq) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nseg) return;
  double tot[2];
  sum_slices<2>(part + (long)i * nsl * 2, nsl, tot);
  seg[i] = tot[0];
  if (csq && i > 0) csq[i - 1] = tot[1];
}

// one interior element: g = w + lambda (2 p - p_prev - p_next) in fp64, out = fl32(p - eta g); eta == 0 hands p through (p - 0 g would turn a -0 into +0)
__device__ inline float geo_elem(float p, float pp, float pn, float w, double eta, double lambda, double& g) {
#pragma clang fp contract(off)
  g = (double)w + lambda * ((2.0 * (double)p - (double)pp) - (double)pn);
  return eta == 0.0 ? p : (float)((double)p - eta * g);
}

constexpr int GEO_NV = 5;                   // per slice: xseg, sum W^2, sum g^2, sum (P_out - P)^2, non-finite elements
// workgroup (slice, i), i = 0 .. m: the slice's part of x-segment i (rows i, i+1 of the OLD curve) and, for i >= 1, the sums of interior row i
__global__ __launch_bounds__(ROW_NT) void geodesic_upd_partial_kernel(const float* P, const float* W, long N, double eta, double lambda, double* part) {
  __shared__ double red[ROW_NT / 64];
  const int i = blockIdx.y, t = threadIdx.x;
  const long nsl = gridDim.x;
  const float *pc = P + (long)i * N, *pn = pc + N, *pp = i > 0 ? pc - N : pc, *wr = i > 0 ? W + (long)(i - 1) * N : pc;
  const bool alc = aligned16(pc), aln = aligned16(pn), alp = aligned16(pp), alw = aligned16(wr);
  double sx = 0.0, sw = 0.0, sg = 0.0, sd = 0.0, bad = 0.0;
#pragma unroll
  for (int gq = 0; gq < ROW_GROUPS; ++gq) {
    const long j = (long)blockIdx.x * ROW_SLICE + ((long)gq * ROW_NT + t) * 4;
    if (j >= N) continue;
    const float4 c4 = row_load4(pc, j, N, alc), n4 = row_load4(pn, j, N, aln);
    const float ci[4] = {c4.x, c4.y, c4.z, c4.w}, ni[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
    for (int c = 0; c < 4; ++c)
      geo_add_sq(sx, (double)ni[c] - (double)ci[c]);
    if (i > 0) {
      const float4 p4 = row_load4(pp, j, N, alp), w4 = row_load4(wr, j, N, alw);
      const float pi[4] = {p4.x, p4.y, p4.z, p4.w}, wi[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        double g;
        const float o = geo_elem(ci[c], pi[c], ni[c], wi[c], eta, lambda, g);
        geo_add_sq(sw, (double)wi[c]);
        geo_add_sq(sg, g);
        geo_add_sq(sd, (double)o - (double)ci[c]);
        if (!geo_finite(ci[c]) || !geo_finite(pi[c]) || !geo_finite(ni[c]) || !geo_finite(wi[c])) bad += 1.0;
      }
    }
  }
  sx = block_sum<ROW_NT>(sx, red);
  sw = block_sum<ROW_NT>(sw, red);
  sg = block_sum<ROW_NT>(sg, red);
  sd = block_sum<ROW_NT>(sd, red);
  bad = block_sum<ROW_NT>(bad, red);
  if (t == 0) {
    double* p = part + ((long)i * nsl + blockIdx.x) * GEO_NV;
    p[0] = sx; p[1] = sw; p[2] = sg; p[3] = sd; p[4] = bad;
  }
}

// workgroup (slice, r), r = 0 .. m+1: the end rows are copied, an interior row takes its step (NaN when flagged); the workgroup of slice 0 writes
// xseg[r] (r <= m) and the statistics of interior row r
__global__ __launch_bounds__(ROW_NT) void geodesic_upd_apply_kernel(const float* P, const float* W, float* P_out, long N, int m, double eta, double lambda,
                                                                   const double* part, double* stats, double* xseg) {
  __shared__ double row_s[GEO_NV];
  const int r = blockIdx.y, t = threadIdx.x;
  const long nsl = gridDim.x;
  const bool inner = r >= 1 && r <= m;
  if (t == 0 && r <= m) sum_slices<GEO_NV>(part + (long)r * nsl * GEO_NV, nsl, row_s);
  __syncthreads();
  const bool bad = inner && row_s[4] != 0.0;
  const float nanf_ = __builtin_nanf("");
  const float *pc = P + (long)r * N, *pp = inner ? pc - N : pc, *pn = inner ? pc + N : pc, *wr = inner ? W + (long)(r - 1) * N : pc;
  float* po = P_out + (long)r * N;
  const bool alc = aligned16(pc), aln = aligned16(pn), alp = aligned16(pp), alw = aligned16(wr), alo = aligned16(po);
#pragma unroll
  for (int gq = 0; gq < ROW_GROUPS; ++gq) {
    const long j = (long)blockIdx.x * ROW_SLICE + ((long)gq * ROW_NT + t) * 4;
    if (j >= N) continue;
    const float4 c4 = row_load4(pc, j, N, alc);
    if (!inner) { row_store4(po, j, N, alo, c4); continue; }
    const float4 n4 = row_load4(pn, j, N, aln), p4 = row_load4(pp, j, N, alp), w4 = row_load4(wr, j, N, alw);
    const float ci[4] = {c4.x, c4.y, c4.z, c4.w}, ni[4] = {n4.x, n4.y, n4.z, n4.w}, pi[4] = {p4.x, p4.y, p4.z, p4.w}, wi[4] = {w4.x, w4.y, w4.z, w4.w};
    float o[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double g;
      o[c] = geo_elem(ci[c], pi[c], ni[c], wi[c], eta, lambda, g);
      if (bad) o[c] = nanf_;
    }
    row_store4(po, j, N, alo, make_float4(o[0], o[1], o[2], o[3]));
  }
  if (t == 0 && blockIdx.x == 0 && r <= m) {
    xseg[r] = row_s[0];
    if (inner) {
      double* st = stats + (long)(r - 1) * 4;
      st[0] = row_s[1]; st[1] = row_s[2]; st[2] = row_s[3]; st[3] = bad ? 1.0 : 0.0;
    }
  }
}

int check_curve(const char* who, long m, long N) {
  if (m < 1 || m + 2 > GEO_MAX_POINTS) { set_error("%s: m=%ld interior points outside [1, %ld]", who, m, GEO_MAX_POINTS - 2); return -1; }
  return check_rows(who, m + 2, N);
}

size_t curve_partial_bytes(long m, long N, int nv) {
  if (m < 1 || m + 2 > GEO_MAX_POINTS || N < 1) return 0;
  return (size_t)(m + 1) * (size_t)row_slices(N) * nv * sizeof(double);
}

}  // namespace

size_t geodesic_cotangents_scratch_bytes(long m, long D) { return curve_partial_bytes(m, D, 2); }
size_t geodesic_update_scratch_bytes(long m, long N) { return curve_partial_bytes(m, N, GEO_NV); }

int launch_geodesic_cotangents(const float* h, float* cot, double* seg, double* csq, long m, long D, void* scratch, size_t scratch_bytes, hipStream_t st) {
  if (check_curve("geodesic_cotangents", m, D)) return -1;
  const size_t need = geodesic_cotangents_scratch_bytes(m, D);
  if (scratch_bytes < need) {
    set_error("geodesic_cotangents: scratch of %zu bytes, dpb_geodesic_cotangents_scratch_bytes(%ld, %ld) = %zu", scratch_bytes, m, D, need);
    return -1;
  }
  if ((uintptr_t)scratch & 7 || (uintptr_t)seg & 7 || (uintptr_t)csq & 7) { set_error("geodesic_cotangents: scratch, seg and csq must be 8-byte aligned"); return -1; }
  const long nsl = row_slices(D);
  double* part = (double*)scratch;
  DPB_LAUNCH(geodesic_cot_kernel, dim3((unsigned)nsl, (unsigned)(m + 1)), dim3(ROW_NT), 0, st, h, D, cot, part);
  DPB_LAUNCH(geodesic_cot_finish_kernel, dim3((unsigned)((m + 1 + 63) / 64)), dim3(64), 0, st, (const double*)part, nsl, (int)(m + 1), seg, csq);
  DPB_CHECK(hipGetLastError());
  return 0;
}

int launch_geodesic_update(const float* P, const float* W, float* P_out, float eta, float lambda, long m, long N, double* stats, double* xseg,
                           void* scratch, size_t scratch_bytes, hipStream_t st) {
  if (check_curve("geodesic_update", m, N)) return -1;
  if (!std::isfinite(eta) || !std::isfinite(lambda) || lambda < 0.f) {
    set_error("geodesic_update: eta=%g and lambda=%g must be finite, lambda >= 0", eta, lambda);
    return -1;
  }
  const size_t need = geodesic_update_scratch_bytes(m, N);
  if (scratch_bytes < need) {
    set_error("geodesic_update: scratch of %zu bytes, dpb_geodesic_update_scratch_bytes(%ld, %ld) = %zu", scratch_bytes, m, N, need);
    return -1;
  }
  if ((uintptr_t)scratch & 7 || (uintptr_t)stats & 7 || (uintptr_t)xseg & 7) { set_error("geodesic_update: scratch, stats and xseg must be 8-byte aligned"); return -1; }
  const uintptr_t a = (uintptr_t)P, b = (uintptr_t)P_out, len = (uintptr_t)(m + 2) * (uintptr_t)N * sizeof(float);
  if (a < b + len && b < a + len) { set_error("geodesic_update: P_out overlaps P: a row reads its neighbours' old values"); return -1; }
  const long nsl = row_slices(N);
  double* part = (double*)scratch;
  DPB_LAUNCH(geodesic_upd_partial_kernel, dim3((unsigned)nsl, (unsigned)(m + 1)), dim3(ROW_NT), 0, st, P, W, N, (double)eta, (double)lambda, part);
  DPB_LAUNCH(geodesic_upd_apply_kernel, dim3((unsigned)nsl, (unsigned)(m + 2)), dim3(ROW_NT), 0, st, P, W, P_out, N, (int)m, (double)eta, (double)lambda,
             (const double*)part, stats, xseg);
  DPB_CHECK(hipGetLastError());
  return 0;
}

}  // namespace dpb
