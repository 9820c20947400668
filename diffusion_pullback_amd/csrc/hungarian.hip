// The Hungarian-matched mean of local bases (run_edit_global_hungarian_mean_zt, src/modules/edit.py:1249-1514; the reference calls a
// compute_hungarian_basis it never defines): the k directions of every basis are matched one to one, and sign by sign, to an anchor's directions and
// the matched unit vectors are averaged.  X [B][k][N] fp32, everything between in fp64.  Two kernels are new here:
//
//   lap_kernel<KMAX>  the batched linear-assignment solver: one workgroup per k x k problem, the shortest-augmenting-path (Jonker-Volgenant) method in
//                     fp64.  The cost matrix, the row duals, the predecessors and both matchings live in LDS (8 k^2 bytes of cost: 32 KiB in the
//                     k <= 64 instantiation, 128 KiB in the k <= 128 one); column j belongs to thread j, which keeps its dual, its shortest-path value
//                     and its scanned flag in registers.  A Dijkstra step is one relaxation of all unscanned columns and one (value, index) arg-min
//                     over the workgroup that breaks ties on the LOWEST column index, so the assignment is a function of the matrix alone.
//                     The matrix is either given (dpb_linear_assignment) or formed while it is loaded from the overlaps of one sweep:
//                     c = G / (||y_i|| ||x_j||), d = 1 / max(|c|, 2^-40) or 1 - |c| (dpb_matched_mean).
//   mean_kernel       one pass over X: a workgroup owns row i of the mean and 1024 columns, walks b = 0 .. B-1 in order, reads row perm[b][i] of basis b
//                     and adds sign / ||x|| times it to fp64 accumulators; the sums go to scratch with the workgroup's partial sum of squares, and
//                     finish_kernel adds the partials in chunk order, divides and rounds to fp32 once.
// The overlaps come from the exact fp64 cross-Gram of angles.hip and the row sums of squares from the fixed-order reduction of transport.hip.
// Reproducibility: no atomics; every sum is one fixed chain.  Workgroup b of lap_kernel reads nothing but problem b.
#include "kernels.h"
#include "geom.h"

#include <cmath>

namespace dpb {

constexpr int HM_NT = 256;                 // threads per workgroup of the mean kernels
constexpr int HM_CHUNK = HM_NT * 4;        // columns per workgroup: four per thread
constexpr int HM_TILE = 256;               // bases whose (row, scale) pairs sit in LDS at a time
constexpr long HM_MAX_BASES = 1L << 20;
constexpr long HM_MAX_ROWS = 1L << 24;     // B k
constexpr double HM_MIN_COS = 0x1p-40;     // the floor of |c| under '1/cosine'

struct LapArgs {
  // a given matrix (G == nullptr) ...
  const double* cost;                      // [B][k][k]
  // ... or the overlaps of a sweep
  const double* G;                         // [k][B k]: <anchor_i, x_{b,j}>
  const double* ssa; const double* ssx;    // [k], [B k]: sums of squares of the anchor's and of the members' rows
  int distance;                            // 0: 1 / max(|c|, 2^-40), 1: 1 - |c|
  int32_t* col_of_row;                     // [B][k] out (the sweep: in as the previous assignment)
  double* total;                           // [B] out
  int32_t* sign;                           // [B][k] in / out (the sweep only)
  double* flag;                            // [B] out (the sweep only): 1 for a degenerate basis
  int32_t* msrc; double* mscale;           // [k][B] out (the sweep only): the row of basis b that feeds row i of the mean, and sign / ||that row||
  int32_t* changed;                        // [B] out (the sweep only): entries (b, i) whose perm or sign differs from the previous one
  long B; int k;
};

__device__ inline bool hm_bad_ss(double s) { return !(s > 0.0) || !(s < 1.7e308); }

// One workgroup of KMAX threads per problem.  Follows the augmenting-row formulation of D. F. Crouse, "On implementing 2D rectangular assignment
// algorithms" (2016): for every row in turn a Dijkstra search over the columns on the reduced costs, the dual update, the augmentation.
template <int KMAX>
__global__ __launch_bounds__(KMAX) void lap_kernel(LapArgs a) {
  constexpr int NW = KMAX / 64;
  __shared__ double cost[KMAX * KMAX];     // row stride k: thread j reads cost[i k + j], consecutive 8-byte words across the lanes
  __shared__ double u[KMAX];               // row duals
  __shared__ int c4r[KMAX], r4c[KMAX], path[KMAX];
  __shared__ double redv[2][NW];
  __shared__ int redi[2][NW];
  const int k = a.k, j = threadIdx.x, lane = j & 63, wave = j >> 6;
  const long b = blockIdx.x;
  const bool sweep = a.G != nullptr;
  const long R = a.B * k;
  const double nan_ = nan64(), inf_ = __longlong_as_double(0x7ff0000000000000LL);

  // ---- the matrix
  int bad = 0;
  double ssx_j = 1.0;
  if (sweep && j < k) { ssx_j = a.ssx[b * k + j]; bad |= hm_bad_ss(ssx_j); }
  if (j < k) {
    const double rx = sqrt(ssx_j);
    for (int i = 0; i < k; ++i) {
      double d;
      if (sweep) {
        const double sa = a.ssa[i];
        bad |= hm_bad_ss(sa);
        const double c = fabs(a.G[(long)i * R + b * k + j] / (sqrt(sa) * rx));
        d = a.distance == 0 ? 1.0 / (c > HM_MIN_COS ? c : HM_MIN_COS) : 1.0 - c;
      } else {
        d = a.cost[(b * k + i) * k + j];
      }
      if (!(fabs(d) < inf_)) bad = 1;
      cost[i * k + j] = d;
    }
  }
  u[j] = 0.0; c4r[j] = -1; r4c[j] = -1; path[j] = -1;
  bad = __syncthreads_or(bad);

  // ---- the assignment
  double v = 0.0;                          // this column's dual
  for (int cur = 0; cur < k && !bad; ++cur) {
    double sh = inf_;                      // this column's shortest-path value
    bool sc = false;                       // this column has been scanned
    int i = cur, sink = -1, step = 0;
    double minv = 0.0;
    while (true) {
      if (j < k && !sc) {
        const double r = minv + cost[i * k + j] - u[i] - v;
        if (r < sh) { sh = r; path[j] = i; }
      }
      double val = (j < k && !sc) ? sh : inf_;
      int idx = j;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(val, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (ov < val || (ov == val && oi < idx)) { val = ov; idx = oi; }
      }
      if (NW > 1) {                        // (two slots: a wave one step ahead writes the other one)
        const int p = step & 1;
        if (lane == 0) { redv[p][wave] = val; redi[p][wave] = idx; }
        __syncthreads();
        val = redv[p][0]; idx = redi[p][0];
#pragma unroll
        for (int w = 1; w < NW; ++w) {
          const double ov = redv[p][w];
          const int oi = redi[p][w];
          if (ov < val || (ov == val && oi < idx)) { val = ov; idx = oi; }
        }
      }
      if (!(val < inf_)) { bad = 1; break; }          // (finite costs whose sums overflowed; uniform: every thread holds the same val)
      minv = val;
      if (j == idx) sc = true;
      const int r = r4c[idx];
      if (r < 0) { sink = idx; break; }
      i = r;
      ++step;
    }
    if (bad) break;
    // duals: the scanned columns and the rows matched to them (the sink has sh == minv and no row), then the new row
    if (j < k && sc) {
      const double d = minv - sh;
      const int r = r4c[j];
      if (r >= 0) u[r] += d;
      v -= d;
    }
    if (j == 0) u[cur] += minv;
    __syncthreads();
    if (j == 0) {                          // augment along the predecessors, from the sink back to cur
      int jj = sink;
      for (int it = 0; it < k; ++it) {       // (a path visits a row once)
        const int ii = path[jj];
        r4c[jj] = ii;
        const int t = c4r[ii];
        c4r[ii] = jj;
        jj = t;
        if (ii == cur) break;
      }
    }
    __syncthreads();
  }

  // ---- results
  if (j == 0) {
    double s = 0.0;
    for (int i = 0; i < k; ++i) s += cost[i * k + (bad ? 0 : c4r[i])];
    a.total[b] = bad ? nan_ : s;
    if (sweep) a.flag[b] = bad ? 1.0 : 0.0;
  }
  int ch = 0;
  if (j < k) {
    const int i = j;                       // from here a thread serves ROW j
    const int col = bad ? -1 : c4r[i];
    const long at = b * k + i;
    if (sweep) {
      int sg = 0;
      double scale = nan_;
      if (!bad) {
        sg = a.G[(long)i * R + b * k + col] < 0.0 ? -1 : 1;
        scale = (double)sg / sqrt(a.ssx[b * k + col]);
      }
      ch = (a.col_of_row[at] != col || a.sign[at] != sg) ? 1 : 0;
      a.sign[at] = sg;
      a.msrc[(long)i * a.B + b] = bad ? 0 : col;
      a.mscale[(long)i * a.B + b] = scale;
    }
    a.col_of_row[at] = col;
  }
  if (sweep) {
    ch = __syncthreads_count(ch);
    if (j == 0) a.changed[b] = ch;
  }
}

// grid (chunks of N, k).  W[i][n] = sum_b mscale[i][b] X[b][msrc[i][b]][n], b in order, one fma per term; part[i][chunk] = the sum of squares of the W
// written.  Four rows are in flight per thread (the loads of a group of four bases are issued before the first is used).
__global__ __launch_bounds__(HM_NT) void mean_kernel(const float* X, const int32_t* msrc, const double* mscale, long B, int k, long N, long chunks,
                                                     double* W, double* part, int vec) {
  __shared__ int src_s[HM_TILE];
  __shared__ double sc_s[HM_TILE];
  __shared__ double red[HM_NT / 64];
  const int i = blockIdx.y, t = threadIdx.x;
  const long chunk = blockIdx.x, n = chunk * HM_CHUNK + (long)t * 4;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (long b0 = 0; b0 < B; b0 += HM_TILE) {
    __syncthreads();                                                 // the previous tile's reads are over
    if (b0 + t < B) { src_s[t] = msrc[(long)i * B + b0 + t]; sc_s[t] = mscale[(long)i * B + b0 + t]; }
    __syncthreads();
    const int nb = B - b0 < HM_TILE ? (int)(B - b0) : HM_TILE;
    for (int bb = 0; bb < nb; bb += 4) {
      float4 x[4];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (bb + q < nb) x[q] = load4(X + ((b0 + bb + q) * k + src_s[bb + q]) * N, n, N, vec);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (bb + q < nb) {
          const double s = sc_s[bb + q];
          a0 = fma(s, (double)x[q].x, a0);
          a1 = fma(s, (double)x[q].y, a1);
          a2 = fma(s, (double)x[q].z, a2);
          a3 = fma(s, (double)x[q].w, a3);
        }
    }
  }
  double* o = W + (long)i * N;                                       // columns past N hold zeros: they add nothing and are not stored
  if (n < N) o[n] = a0;
  if (n + 1 < N) o[n + 1] = a1;
  if (n + 2 < N) o[n + 2] = a2;
  if (n + 3 < N) o[n + 3] = a3;
  double s = a0 * a0;
  s += a1 * a1;
  s += a2 * a2;
  s += a3 * a3;
  s = block_sum<HM_NT>(s, red);
  if (t == 0) part[(long)i * chunks + chunk] = s;
}

// grid (chunks of N, k): Y[i] = W[i] / sqrt(the chunks' partial sums in chunk order), rounded to fp32 once (W = 0 gives NaN; NaN stays NaN)
__global__ __launch_bounds__(HM_NT) void finish_kernel(const double* W, const double* part, long N, long chunks, float* Y, int vec) {
  __shared__ double norm_s;
  const int i = blockIdx.y;
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (long c = 0; c < chunks; ++c) s += part[(long)i * chunks + c];
    norm_s = sqrt(s);
  }
  __syncthreads();
  const double nrm = norm_s;
  const long n = (long)blockIdx.x * HM_CHUNK + (long)threadIdx.x * 4;
  if (n >= N) return;
  const double* w = W + (long)i * N + n;
  float* y = Y + (long)i * N + n;
  if (vec) {
    *reinterpret_cast<float4*>(y) = make_float4((float)(w[0] / nrm), (float)(w[1] / nrm), (float)(w[2] / nrm), (float)(w[3] / nrm));
  } else {
    for (int e = 0; e < 4 && n + e < N; ++e) y[e] = (float)(w[e] / nrm);
  }
}

// one workgroup: info[0] = the number of (b, i) entries that changed (a sum of integers: any order gives the same)
__global__ __launch_bounds__(HM_NT) void changed_kernel(const int32_t* changed, long B, double* info) {
  __shared__ double red[HM_NT / 64];
  double c = 0.0;
  for (long b = threadIdx.x; b < B; b += HM_NT) c += (double)changed[b];
  c = block_sum<HM_NT>(c, red);
  if (threadIdx.x == 0) info[0] = c;
}

// ------------------------------------------------------------------------------------------------------------ host side
static void lap_launch(const LapArgs& a, hipStream_t st) {
  if (a.k <= 64) DPB_LAUNCH((lap_kernel<64>), dim3((unsigned)a.B), dim3(64), 0, st, a);
  else DPB_LAUNCH((lap_kernel<HUNGARIAN_MAX_RANK>), dim3((unsigned)a.B), dim3(HUNGARIAN_MAX_RANK), 0, st, a);
}

size_t linear_assignment_scratch_bytes(long B, int k) {
  if (B < 1 || B > HM_MAX_BASES || k < 1 || k > HUNGARIAN_MAX_RANK) return 0;
  return 256;                                                        // (the solver keeps its whole state in LDS; the block is reserved)
}

int launch_linear_assignment(const double* cost, long B, int k, int32_t* col_of_row, double* total, void* scratch, size_t scratch_bytes, hipStream_t st) {
  const size_t need = linear_assignment_scratch_bytes(B, k);
  if (!need) { set_error("dpb_linear_assignment: B=%ld outside [1,%ld] or k=%d outside [1,%d]", B, HM_MAX_BASES, k, HUNGARIAN_MAX_RANK); return -1; }
  if (check_scratch("dpb_linear_assignment", scratch, scratch_bytes, need, "dpb_linear_assignment_scratch_bytes(%ld, %d)", B, k) != 0) return -1;
  LapArgs a{};
  a.cost = cost; a.col_of_row = col_of_row; a.total = total; a.B = B; a.k = k;
  lap_launch(a, st);
  DPB_CHECK(hipGetLastError());
  return 0;
}

namespace {
struct MeanLayout { size_t g = 0, ssa = 0, ssx = 0, msrc = 0, mscale = 0, changed = 0, w = 0, part = 0, total = 0; long chunks = 0; };
bool mean_layout(long B, int k, long N, MeanLayout& l) {
  if (B < 1 || B > HM_MAX_BASES || k < 1 || k > HUNGARIAN_MAX_RANK || N < 1 || B * k > HM_MAX_ROWS) return false;
  ScratchCarver s;
  l.chunks = (N + HM_CHUNK - 1) / HM_CHUNK;
  if (l.chunks > 0x7fffffffL) return false;
  l.g = s.take((size_t)k * B * k * sizeof(double));
  l.ssa = s.take((size_t)k * sizeof(double));
  l.ssx = s.take((size_t)B * k * sizeof(double));
  l.msrc = s.take((size_t)B * k * sizeof(int32_t));
  l.mscale = s.take((size_t)B * k * sizeof(double));
  l.changed = s.take((size_t)B * sizeof(int32_t));
  l.w = s.take((size_t)k * N * sizeof(double));
  l.part = s.take((size_t)k * (size_t)l.chunks * sizeof(double));
  l.total = s.off;
  return true;
}
}  // namespace

size_t matched_mean_scratch_bytes(long B, int k, long N) {
  MeanLayout l;
  return mean_layout(B, k, N, l) ? l.total : 0;
}

int launch_matched_mean(const float* X, long B, int k, long N, const float* anchor, int init, int distance, float* Y, int32_t* perm, int32_t* sign,
                        double* info, void* scratch, size_t scratch_bytes, hipStream_t st) {
  MeanLayout l;
  if (!mean_layout(B, k, N, l)) {
    set_error("dpb_matched_mean: B=%ld outside [1,%ld], k=%d outside [1,%d], N=%ld < 1 or B k above %ld", B, HM_MAX_BASES, k, HUNGARIAN_MAX_RANK, N,
              HM_MAX_ROWS);
    return -1;
  }
  if (!anchor && (init < 0 || init >= B)) { set_error("dpb_matched_mean: init=%d outside [0,%ld)", init, B); return -1; }
  if (distance != 0 && distance != 1) { set_error("dpb_matched_mean: distance=%d is neither 0 (1/cosine) nor 1 (cosine)", distance); return -1; }
  if (check_scratch("dpb_matched_mean", scratch, scratch_bytes, l.total, "dpb_matched_mean_scratch_bytes(%ld, %d, %ld)", B, k, N) != 0) return -1;
  if (!anchor) anchor = X + (long)init * k * N;
  char* base = (char*)scratch;
  double* G = (double*)(base + l.g);
  double* ssa = (double*)(base + l.ssa);
  double* ssx = (double*)(base + l.ssx);
  int32_t* msrc = (int32_t*)(base + l.msrc);
  double* mscale = (double*)(base + l.mscale);
  int32_t* changed = (int32_t*)(base + l.changed);
  double* W = (double*)(base + l.w);
  double* part = (double*)(base + l.part);
  // the overlaps: an entry of the cross-Gram does not depend on the rows around it, so basis b's block is the same in any stack
  if (launch_cross_gram(anchor, X, G, k, (int)(B * k), N, st) != 0) return -1;
  if (launch_rowsumsq(anchor, k, N, ssa, st) != 0) return -1;
  if (launch_rowsumsq(X, B * k, N, ssx, st) != 0) return -1;
  LapArgs a{};
  a.G = G; a.ssa = ssa; a.ssx = ssx; a.distance = distance; a.col_of_row = perm; a.total = info + 1; a.sign = sign; a.flag = info + 1 + B;
  a.msrc = msrc; a.mscale = mscale; a.changed = changed; a.B = B; a.k = k;
  lap_launch(a, st);
  DPB_LAUNCH(changed_kernel, dim3(1), dim3(HM_NT), 0, st, changed, B, info);
  const int vx = (N % 4 == 0 && (uintptr_t)X % 16 == 0) ? 1 : 0, vy = (N % 4 == 0 && (uintptr_t)Y % 16 == 0) ? 1 : 0;
  DPB_LAUNCH(mean_kernel, dim3((unsigned)l.chunks, (unsigned)k), dim3(HM_NT), 0, st, X, msrc, mscale, B, k, N, l.chunks, W, part, vx);
  DPB_LAUNCH(finish_kernel, dim3((unsigned)l.chunks, (unsigned)k), dim3(HM_NT), 0, st, W, part, N, l.chunks, Y, vy);
  DPB_CHECK(hipGetLastError());
  return 0;
}

}  // namespace dpb
