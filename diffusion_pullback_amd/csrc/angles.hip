// Principal angles and Grassmann geodesic distances between stacks of k-dimensional subspaces of R^N (the saved local tangent spaces u / vT of
// run_sample_encoder_local_tangent_space_zt; k <= 128, N up to 196 608, hundreds of bases), fp32 in / fp32 out, everything between in fp64.
//
// Nothing of size N is orthonormalised or written.  One streaming pass forms the cross-Gram of all rows on the fp64 matrix cores
// (v_mfma_f64_16x16x4_f64: the fp32 inputs are widened on load, so every product is exact and only the fp64 accumulation rounds); the rest is small
// dense algebra per basis and per pair:
//   per basis i:  d = diag(G_ii), Ghat_ii = D^-1/2 G_ii D^-1/2 = L_i L_i^T (Cholesky), W_i = L_i^-1 D^-1/2          (prep_kernel)
//   per pair i,j: M = W_i G_ij W_j^T (the cosines are its singular values), S = I - M M^T (the Schur complement of the whitened joint Gram: its
//                 eigenvalues are sin^2 theta), Jacobi eigenvalues of S, theta = asin(sqrt(l)) for l <= 1/2, else acos(sqrt(1 - l))   (pair_kernel)
// The sine comes from a difference of exactly accumulated Gram entries, so small angles keep their relative accuracy, where acos of a cosine next
// to 1 has lost it.
// Reproducibility: no atomics.  Every Gram entry is one fixed chain of additions -- the k order inside a slice of N, then the slices in slice order,
// both functions of N only -- so an entry does not depend on the number of rows, on the tile it falls in or on the launch; the small algebra sums
// sequentially per element.  theta of a pair is therefore a function of the 2k rows of the pair and of N, bitwise.
#include "kernels.h"
#include "geom.h"

namespace dpb {

typedef double gram_d4 __attribute__((ext_vector_type(4)));

constexpr int GT = 64;        // rows x rows of G per workgroup (four waves, 32 x 32 each: 2 x 2 MFMA tiles)
constexpr int GK = 32;        // columns of N per LDS stage
constexpr int GS = GK + 4;    // LDS row stride in floats: 16 rows x 36 words fall on 16 distinct groups of four banks (the 16-byte fragment reads are conflict-free)

// the slice of N one launch adds to G: at most eight slices, whole LDS stages; a function of N ONLY (batch invariance)
static inline long gram_slice(long N) {
  long s = (N + 7) / 8;
  s = (s + GK - 1) / GK * GK;
  return s < 4096 ? 4096 : s;
}

struct GramArgs {
  const float* X; const float* Y; double* G;
  int Ra, Rb;               // rows of X, of Y (per batch entry)
  long N, ldg;              // row length of X and Y; row stride of G
  long n0, n1;              // this launch's slice of N
  long bx, by, bg;          // batch strides (blockIdx.z) of X, Y, G in elements
  int self, first, vec;     // self: Y == X, only tiles ti <= tj are computed and mirrored; first: store instead of add; vec: 16-byte loads are legal
};

__device__ inline float4 gram_load(const float* P, int R, long N, int row, long col, long n1, int vec) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (row < R && col < n1) {
    const float* p = P + (long)row * N + col;
    if (vec) {
      v = *reinterpret_cast<const float4*>(p);       // (vec: N % 4 == 0, col % 4 == 0 and n1 % 4 == 0, so col + 3 < n1)
    } else {
      v.x = p[0];
      if (col + 1 < n1) v.y = p[1];
      if (col + 2 < n1) v.z = p[2];
      if (col + 3 < n1) v.w = p[3];
    }
  }
  return v;
}

// grid (tiles of Rb, tiles of Ra, batch).  Lane l of a wave holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15] of v_mfma_f64_16x16x4_f64;
// here lane (r, g) reads the FOUR columns 4g .. 4g+3 of its row in one 16-byte LDS access and feeds element e to MFMA e of the group: a permutation of
// k that is the same for both operands.  C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 * reg (not the f32 map).
__global__ __launch_bounds__(256) void cross_gram_kernel(GramArgs a) {
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (a.self && ti > tj) return;
  const float* X = a.X + (long)blockIdx.z * a.bx;
  const float* Y = a.Y + (long)blockIdx.z * a.by;
  double* G = a.G + (long)blockIdx.z * a.bg;
  __shared__ __attribute__((aligned(16))) float xs[GT * GS], ys[GT * GS];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wr = wave >> 1, wc = wave & 1;
  const int lrow = t >> 3, lq = (t & 7) * 4;     // this thread's staging: rows lrow, lrow + 32, columns lq .. lq + 3 of the stage
  gram_d4 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) acc[m][n] = gram_d4{0.0, 0.0, 0.0, 0.0};
  float4 px[2], py[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    px[u] = gram_load(X, a.Ra, a.N, ti * GT + lrow + 32 * u, a.n0 + lq, a.n1, a.vec);
    py[u] = gram_load(Y, a.Rb, a.N, tj * GT + lrow + 32 * u, a.n0 + lq, a.n1, a.vec);
  }
  for (long n = a.n0; n < a.n1; n += GK) {
    __syncthreads();                               // the previous stage's fragment reads are done
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      *reinterpret_cast<float4*>(&xs[(lrow + 32 * u) * GS + lq]) = px[u];
      *reinterpret_cast<float4*>(&ys[(lrow + 32 * u) * GS + lq]) = py[u];
    }
    __syncthreads();
    if (n + GK < a.n1) {                           // the next stage's loads fly under this stage's MFMAs
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        px[u] = gram_load(X, a.Ra, a.N, ti * GT + lrow + 32 * u, n + GK + lq, a.n1, a.vec);
        py[u] = gram_load(Y, a.Rb, a.N, tj * GT + lrow + 32 * u, n + GK + lq, a.n1, a.vec);
      }
    }
#pragma unroll
    for (int kk = 0; kk < GK; kk += 16) {
      float4 af[2], bf[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        af[m] = *reinterpret_cast<const float4*>(&xs[(wr * 32 + m * 16 + (lane & 15)) * GS + kk + 4 * (lane >> 4)]);
        bf[m] = *reinterpret_cast<const float4*>(&ys[(wc * 32 + m * 16 + (lane & 15)) * GS + kk + 4 * (lane >> 4)]);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double a0 = (double)(e == 0 ? af[0].x : e == 1 ? af[0].y : e == 2 ? af[0].z : af[0].w);
        const double a1 = (double)(e == 0 ? af[1].x : e == 1 ? af[1].y : e == 2 ? af[1].z : af[1].w);
        const double b0 = (double)(e == 0 ? bf[0].x : e == 1 ? bf[0].y : e == 2 ? bf[0].z : bf[0].w);
        const double b1 = (double)(e == 0 ? bf[1].x : e == 1 ? bf[1].y : e == 2 ? bf[1].z : bf[1].w);
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
  }
  // G (+)= this slice, in slice order: the launches of one call are stream-ordered and each element belongs to one thread of one workgroup
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = ti * GT + wr * 32 + m * 16 + (lane >> 4) + 4 * r;
        const int gj = tj * GT + wc * 32 + n * 16 + (lane & 15);
        if (gi < a.Ra && gj < a.Rb) {
          const long at = (long)gi * a.ldg + gj;
          double v = acc[m][n][r];
          if (!a.first) v = G[at] + v;
          G[at] = v;
          if (a.self && ti != tj) G[(long)gj * a.ldg + gi] = v;       // mirror of an off-diagonal tile (a diagonal tile computes both halves itself)
        }
      }
}

static int gram_launches(const float* X, const float* Y, double* G, int Ra, int Rb, long N, long ldg, int batch, long bx, long by, long bg, int self,
                         hipStream_t st) {
  GramArgs a;
  a.X = X; a.Y = Y; a.G = G; a.Ra = Ra; a.Rb = Rb; a.N = N; a.ldg = ldg; a.bx = bx; a.by = by; a.bg = bg; a.self = self;
  a.vec = (N % 4 == 0 && (uintptr_t)X % 16 == 0 && (uintptr_t)Y % 16 == 0) ? 1 : 0;      // (batch strides are multiples of N)
  const long sl = gram_slice(N);
  const dim3 grid((Rb + GT - 1) / GT, (Ra + GT - 1) / GT, batch);
  for (long n0 = 0; n0 < N; n0 += sl) {
    a.n0 = n0; a.n1 = n0 + sl < N ? n0 + sl : N; a.first = n0 == 0;
    DPB_LAUNCH(cross_gram_kernel, grid, dim3(256), 0, st, a);
  }
  return 0;
}

int launch_cross_gram(const float* X, const float* Y, double* G, int Ra, int Rb, long N, hipStream_t st) {
  if (Ra < 1 || Rb < 1 || N < 1) { set_error("dpb_cross_gram: Ra=%d, Rb=%d, N=%ld: all must be >= 1", Ra, Rb, N); return -1; }
  if (!Y && Ra != Rb) { set_error("dpb_cross_gram: Y = NULL (Y = X) needs Rb = Ra, got Ra=%d, Rb=%d", Ra, Rb); return -1; }
  if ((Ra + GT - 1) / GT > 65535) { set_error("dpb_cross_gram: Ra=%d above %d rows", Ra, 65535 * GT); return -1; }
  gram_launches(X, Y ? Y : X, G, Ra, Rb, N, Rb, 1, 0, 0, 0, Y ? 0 : 1, st);
  DPB_CHECK(hipGetLastError());
  return 0;
}

// each basis's own Gram block: Dg[b] [k][k] = X_b X_b^T for the n bases of X [n][k][N], one batch entry per basis (the chains of launch_cross_gram: an
// entry is a function of its two rows and N alone); also flagkmeans.hip
int launch_self_gram_blocks(const float* X, double* Dg, int n, int k, long N, hipStream_t st) {
  if (n < 1 || n > 65535 || k < 1 || N < 1) { set_error("self Gram blocks: n=%d outside [1,65535], k=%d or N=%ld below 1", n, k, N); return -1; }
  return gram_launches(X, X, Dg, k, k, N, k, n, (long)k * N, (long)k * N, (long)k * k, 1, st);
}

// ------------------------------------------------------------------------------------------------------------ per basis: whitening
constexpr double ANGLES_MIN_PIVOT = 1e-10;   // smallest Cholesky pivot (the diagonal entry before its square root) of the row-normalised Gram block

// one workgroup per basis: Dg [k][k] (its diagonal Gram block) -> W = L^-1 D^-1/2 in the same slot (lower triangular, zeros above), flag = 1 for a
// degenerate basis (a zero or non-finite row norm, a pivot below ANGLES_MIN_PIVOT or not a number)
template <int KMAX>
__global__ __launch_bounds__(256) void angles_prep_kernel(double* Dg, int* flags, int k) {
  double* D = Dg + (long)blockIdx.x * k * k;
  __shared__ double A[KMAX][KMAX + 1], rs[KMAX], dinv[KMAX];
  __shared__ int bad;
  static_assert(sizeof(double) * (KMAX * (KMAX + 1) + 2 * KMAX) + sizeof(int) <= 160 * 1024, "angles_prep_kernel exceeds the gfx950 LDS");
  const int t = threadIdx.x;
  if (t == 0) bad = 0;
  __syncthreads();
  if (t < k) {
    const double d = D[(long)t * k + t];
    if (!(d > 0.0) || !(d < 1.7e308)) bad = 1;     // (a benign race: every writer stores 1)
    rs[t] = 1.0 / sqrt(d);
  }
  __syncthreads();
  for (int e = t; e < k * k; e += 256) {
    const int i = e / k, j = e % k;
    A[i][j] = D[(long)(i <= j ? i : j) * k + (i <= j ? j : i)] * rs[i] * rs[j];      // the upper half, mirrored: exactly symmetric
  }
  __syncthreads();
  if (!bad) {
    for (int j = 0; j < k; ++j) {                  // right-looking Cholesky, the factor in the lower triangle
      const double piv = A[j][j];
      __syncthreads();
      if (!(piv >= ANGLES_MIN_PIVOT)) { if (t == 0) bad = 1; break; }      // uniform: every thread read the same pivot
      const double l = sqrt(piv);
      for (int r = j + t; r < k; r += 256) A[r][j] = r == j ? l : A[r][j] / l;
      __syncthreads();
      const int m = k - 1 - j;                     // trailing block: rows / columns j+1 .. k-1, lower half
      for (int e = t; e < m * m; e += 256) {
        const int r = j + 1 + e / m, c = j + 1 + e % m;
        if (c <= r) A[r][c] -= A[r][j] * A[c][j];
      }
      __syncthreads();
    }
  }
  __syncthreads();
  if (bad) {
    if (t == 0) flags[blockIdx.x] = 1;
    return;
  }
  if (t == 0) flags[blockIdx.x] = 0;
  // X = L^-1 by forward substitution, thread c owns column c: X[r][c] for r > c goes to A[c][r] (the free upper triangle), X[c][c] to dinv
  if (t < k) {
    const int c = t;
    dinv[c] = 1.0 / A[c][c];
    for (int r = c + 1; r < k; ++r) {
      double s = A[r][c] * dinv[c];
      for (int b = c + 1; b < r; ++b) s += A[r][b] * A[c][b];
      A[c][r] = -s / A[r][r];
    }
  }
  __syncthreads();
  for (int e = t; e < k * k; e += 256) {
    const int r = e / k, c = e % k;
    D[e] = r < c ? 0.0 : (r == c ? dinv[c] : A[c][r]) * rs[c];
  }
}

// the whitening of n bases in place (also the Frechet mean's, frechet.hip): Dg [n][k][k] Gram blocks -> W, flags [n]; 1 <= k <= ORTH_MAX_RANK
void launch_angles_prep(double* Dg, int* flags, int n, int k, hipStream_t st) {
  DPB_BY_RANK128(k, (void)NT; DPB_LAUNCH((angles_prep_kernel<KM>), dim3(n), dim3(256), 0, st, Dg, flags, k));
}

// one workgroup per block b of a stacked Gram: dst[b][r][c] = G[(b rstep + r) ld + b k + c] (launch_gram_blocks, kernels.h; also frechet.hip, geodesic.hip)
__global__ __launch_bounds__(256) void gram_blocks_kernel(const double* G, double* dst, long ld, int rstep, int k) {
  const long b = blockIdx.x;
  for (int e = threadIdx.x; e < k * k; e += 256) dst[b * k * k + e] = G[(b * rstep + e / k) * ld + b * k + e % k];
}

void launch_gram_blocks(const double* G, double* dst, int n, long ld, int rstep, int k, hipStream_t st) {
  DPB_LAUNCH(gram_blocks_kernel, dim3(n), dim3(256), 0, st, G, dst, ld, rstep, k);
}

// ------------------------------------------------------------------------------------------------------------ per pair: angles
// Workgroups walk the pairs p = blockIdx.x, blockIdx.x + gridDim.x, ...; pair (i, j) = (p / Bb, p % Bb).  T = W_i G_ij and M = T W_j^T go through this
// workgroup's two k x k slots of global scratch (L2), S = I - M M^T lives in LDS, its eigenvalues come from a two-sided Jacobi iteration in the round-robin
// order (jacobi_round_robin of geom.h, without eigenvectors).
template <int KMAX, int NT>
__global__ __launch_bounds__(NT) void angles_pair_kernel(const double* Wa, const double* Wb, const int* fa, const int* fb, const double* Gab, long ldg,
                                                         double* work, float* theta, float* dist, int Ba, int Bb, int k, int self) {
  __shared__ double A[KMAX][KMAX + 1];
  __shared__ double lam[KMAX], th[KMAX];
  __shared__ JacobiWs<KMAX> ws;
  static_assert(sizeof(double) * (KMAX * (KMAX + 1) + 2 * KMAX) + sizeof(JacobiWs<KMAX>) <= 160 * 1024, "angles_pair_kernel exceeds the gfx950 LDS");
  const int t = threadIdx.x;
  double* const Tm = work + (long)blockIdx.x * 2 * k * k;
  double* const Mm = Tm + (long)k * k;
  for (long p = blockIdx.x; p < (long)Ba * Bb; p += gridDim.x) {
    const int i = (int)(p / Bb), j = (int)(p % Bb);
    if (self && i > j) continue;
    const bool degenerate = fa[i] != 0 || fb[j] != 0;
    if (degenerate || (self && i == j)) {          // NaN for a degenerate basis's row and column; the self-mode diagonal is exactly 0
      const float v = degenerate ? (float)nan64() : 0.f;
      for (int e = t; e < k; e += NT) {
        theta[((long)i * Bb + j) * k + e] = v;
        if (self) theta[((long)j * Bb + i) * k + e] = v;
      }
      if (t == 0) { dist[(long)i * Bb + j] = v; if (self) dist[(long)j * Bb + i] = v; }
      continue;
    }
    const double* Wi = Wa + (long)i * k * k;
    const double* Wj = Wb + (long)j * k * k;
    const double* Gij = Gab + (long)i * k * ldg + (long)j * k;
    __syncthreads();                               // the previous pair is done with T, M and the LDS
    for (int e = t; e < k * k; e += NT) {          // T = W_i G_ij (W_i lower triangular)
      const int r = e / k, c = e % k;
      double s = 0.0;
      for (int b = 0; b <= r; ++b) s += Wi[r * k + b] * Gij[(long)b * ldg + c];
      Tm[e] = s;
    }
    __syncthreads();
    for (int e = t; e < k * k; e += NT) {          // M = T W_j^T
      const int r = e / k, c = e % k;
      double s = 0.0;
      for (int b = 0; b <= c; ++b) s += Tm[r * k + b] * Wj[c * k + b];
      Mm[e] = s;
    }
    __syncthreads();
    for (int e = t; e < k * k; e += NT) {          // S = I - M M^T, the upper half mirrored
      const int r = e / k, c = e % k;
      if (r <= c) {
        double s = 0.0;
        for (int b = 0; b < k; ++b) s += Mm[r * k + b] * Mm[c * k + b];
        const double v = (r == c ? 1.0 : 0.0) - s;
        A[r][c] = v; A[c][r] = v;
      }
    }
    __syncthreads();
    jacobi_round_robin<KMAX, NT>(A, JacobiNoVecs{}, ws, k);
    if (t < k) {
      const double l = A[t][t];
      lam[t] = l < 0.0 ? 0.0 : (l > 1.0 ? 1.0 : l);          // (a NaN stays a NaN and reaches the output)
    }
    __syncthreads();
    if (t < k) {                                   // descending, NaN first, ties by index: every slot of th is written for any lam (rank.h)
      const double mine = lam[t];
      th[rank_desc(lam, k, t)] = mine <= 0.5 ? asin(sqrt(mine)) : acos(sqrt(1.0 - mine));
    }
    __syncthreads();
    for (int e = t; e < k; e += NT) {
      theta[((long)i * Bb + j) * k + e] = (float)th[e];
      if (self) theta[((long)j * Bb + i) * k + e] = (float)th[e];
    }
    if (t == 0) {
      double s = 0.0;
      for (int e = 0; e < k; ++e) s += th[e] * th[e];
      const float d = (float)sqrt(s);
      dist[(long)i * Bb + j] = d;
      if (self) dist[(long)j * Bb + i] = d;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ host side
constexpr int ANGLES_MAX_BASES = 65535;      // bases per stack (a grid axis of the batched Gram launch)
constexpr long ANGLES_PAIR_BLOCKS = 1024;    // workgroups of the pair kernel (each owns two k x k fp64 slots of scratch)

namespace {
struct AnglesLayout { size_t gab = 0, wa = 0, wb = 0, flags = 0, work = 0, total = 0; long nblk = 0; };
bool angles_layout(long Ba, long Bb, int k, long N, AnglesLayout& l) {
  if (Ba < 1 || Bb < 1 || Ba > ANGLES_MAX_BASES || Bb > ANGLES_MAX_BASES || k < 1 || k > ORTH_MAX_RANK || N < 1 || k > N) return false;
  ScratchCarver s;
  const size_t kk = (size_t)k * k * sizeof(double);
  l.nblk = Ba * Bb < ANGLES_PAIR_BLOCKS ? Ba * Bb : ANGLES_PAIR_BLOCKS;
  l.gab = s.take((size_t)Ba * k * (size_t)Bb * k * sizeof(double));
  l.wa = s.take((size_t)Ba * kk);
  l.wb = s.take((size_t)Bb * kk);
  l.flags = s.take((size_t)(Ba + Bb) * sizeof(int));
  l.work = s.take((size_t)l.nblk * 2 * kk);
  l.total = s.off;
  return true;
}
}  // namespace

size_t subspace_angles_scratch_bytes(long Ba, long Bb, int k, long N) {
  AnglesLayout l;
  return angles_layout(Ba, Bb, k, N, l) ? l.total : 0;
}

int launch_subspace_angles(const float* A, const float* B, long Ba, long Bb, int k, long N, float* theta, float* dist, void* scratch,
                           size_t scratch_bytes, hipStream_t st) {
  AnglesLayout l;
  if (!angles_layout(Ba, Bb, k, N, l)) {
    set_error("dpb_subspace_angles: Ba=%ld, Bb=%ld outside [1,%d], k=%d outside [1,%d], or N=%ld < k", Ba, Bb, ANGLES_MAX_BASES, k, ORTH_MAX_RANK, N);
    return -1;
  }
  const bool self = B == nullptr;
  if (self && Ba != Bb) { set_error("dpb_subspace_angles: B = NULL (self mode) needs Bb = Ba, got Ba=%ld, Bb=%ld", Ba, Bb); return -1; }
  if (check_scratch("dpb_subspace_angles", scratch, scratch_bytes, l.total, "dpb_subspace_angles_scratch_bytes(%ld, %ld, %d, %ld)", Ba, Bb, k, N) != 0) return -1;
  if ((Ba * k + GT - 1) / GT > 65535) { set_error("dpb_subspace_angles: Ba * k = %ld above %d rows", Ba * k, 65535 * GT); return -1; }
  char* base = (char*)scratch;
  double* Gab = (double*)(base + l.gab);
  double* Wa = (double*)(base + l.wa);
  double* Wb = self ? Wa : (double*)(base + l.wb);
  int* fa = (int*)(base + l.flags);
  int* fb = self ? fa : fa + Ba;
  double* work = (double*)(base + l.work);
  const int Ra = (int)(Ba * k), Rb = (int)(Bb * k), sf = self ? 1 : 0;
  // the cross block of every pair (self mode: the tiles on and above the diagonal, mirrored; the block of a pair i < j lies above it) ...
  gram_launches(A, self ? A : B, Gab, Ra, Rb, N, Rb, 1, 0, 0, 0, sf, st);
  // ... and each basis's own k x k block, one batch entry per basis, into the slot its whitening matrix W will take
  gram_launches(A, A, Wa, k, k, N, k, (int)Ba, (long)k * N, (long)k * N, (long)k * k, 1, st);
  if (!self) gram_launches(B, B, Wb, k, k, N, k, (int)Bb, (long)k * N, (long)k * N, (long)k * k, 1, st);
  launch_angles_prep(Wa, fa, (int)Ba, k, st);
  if (!self) launch_angles_prep(Wb, fb, (int)Bb, k, st);
  const dim3 pg((unsigned)l.nblk);
  DPB_BY_RANK128(k, DPB_LAUNCH((angles_pair_kernel<KM, NT>), pg, dim3(NT), 0, st, Wa, Wb, fa, fb, Gab, (long)Rb, work, theta, dist, (int)Ba, (int)Bb, k, sf));
  DPB_CHECK(hipGetLastError());
  return 0;
}

}  // namespace dpb
