// Grassmann geodesics between the row spans of pairs of bases (A_d, B_d), both [k][N] fp32, rows independent but not necessarily orthonormal:
// principal vectors, the log map, points of the geodesic, and the exp map of a tangent given as (P, H).  k <= 64; everything small in fp64.
//
// Nothing of size N is formed before the stream.  Per pair, from the exact fp64 Grams A A^T, B B^T, A B^T (dpb_cross_gram) and the whitenings Wa, Wb
// of angles.hip (W G W^T = I):
//   M = Wa (A B^T) Wb^T;  S = I - M M^T = V sin^2(theta) V^T (Jacobi with vectors);  U = V^T M, row i of norm cos(theta_i);
//   theta = asin(sqrt(lambda)) for lambda <= 1/2, acos ||U_i|| above (the rule of fr_basis_kernel), ordered descending, ties by index;
//   Pa = Ra A, Ra = V^T Wa;  Pb = Rb B, Rb = diag(1 / cos theta) U Wb:  orthonormal rows, Pa Pb^T = diag(cos theta);
//   sign: the entry of largest magnitude of each row of V^T (lowest index on ties) is positive.
// Every output row is alpha_i pa_i + beta_i pb_i:
//   geodesic at t   alpha = sin((1 - t) theta) / sin theta, beta = sin(t theta) / sin theta   (1 - t and t at sin theta = 0);
//   log map         alpha = -theta cos theta / sin theta,   beta = theta / sin theta          (-1 and 1 at sin theta = 0).
// Exp map of (P, H): W the whitening of P, Q = W P, K = (W H) Q^T = W (H P^T) W^T, Hq = W H - K Q, Hq Hq^T = W (H H^T) W^T - K K^T = V sigma^2 V^T;
//   y_i(t) = cos(t sigma_i) (V^T Q)_i + (sin(t sigma_i) / sigma_i) (V^T Hq)_i, with V^T Q = (V^T W) P and V^T Hq = -(V^T K W) P + (V^T W) H.
// The pair kernel leaves the k x k coefficient matrices and the alpha / beta tables; the stream kernel makes ONE pass over the 2k rows of a pair on the
// fp64 matrix cores (fp32 rows widened on load, summed in index order), holds both rotated tiles in registers and writes every output slice from them
// with one multiply and one fma per element, rounded to fp32 once.
// Reproducibility: no atomics, every sum a fixed chain.  A Gram entry is a function of its two rows and N only (angles.hip), so the result of a pair is
// bitwise the same alone, at any position of a stack, and with A broadcast.
#include "../../include/dpb.h"
#include "kernels.h"
#include "geom.h"

namespace dpb {

constexpr double GD_HALF_PI = 1.57079632679489661923;
constexpr double GD_DOMAIN = GD_HALF_PI - 1e-6;      // FR_DOMAIN of frechet.hip: beyond it the geodesic is not unique and 1 / cos theta is unbounded
constexpr int GD_MAX_SLICES = 64;                    // output slices (values of t) per call: they travel as kernel arguments
constexpr int GD_MAX_PAIRS = 65535;                  // a grid axis
constexpr int GD_CHUNK_ROWS = 512;                   // rows per stacked Gram call

enum { GD_VECTORS = 0, GD_LOG = 1, GD_GEODESIC = 2, GD_EXP = 3 };

struct GdTs { double t[GD_MAX_SLICES]; };

struct GdPairArgs {
  const double* Wa; long wa_stride;      // whitening of A_d (of P_d), 0: one for all pairs
  const double* Wb;                      // whitening of B_d; GD_EXP: the raw Gram H H^T
  const double* Gab;                     // A B^T (P H^T)
  const int* fa; int fa_stride;          // whitening flags
  const int* fb;                         // (not read by GD_EXP)
  double *Z1a, *Z2a, *Z2b;               // coefficient matrices, transposed [source row][output row]; Z2a only GD_EXP
  double *alpha, *beta;                  // [D][S][k]
  float* spec;                           // theta / sigma [D][k]
  int* flags;                            // [D]
  GdTs ts;
  int S, k, mode;
};

// One workgroup per pair (per (P, H)).  LDS: A (the symmetric matrix, then U), V (a product's left factor, then the eigenvectors), Mm (M or K).
template <int KMAX, int NT>
__global__ __launch_bounds__(NT) void gd_pair_kernel(GdPairArgs a) {
  __shared__ double A[KMAX][KMAX + 1], V[KMAX][KMAX + 1], Mm[KMAX][KMAX + 1];
  __shared__ double lam[KMAX], val[KMAX], csv[KMAX], snv[KMAX], sgn[KMAX];
  __shared__ int ord[KMAX];
  __shared__ JacobiWs<KMAX> ws;
  static_assert(sizeof(double) * (3 * KMAX * (KMAX + 1) + 5 * KMAX) + sizeof(int) * KMAX + sizeof(JacobiWs<KMAX>) <= 160 * 1024,
                "gd_pair_kernel exceeds the gfx950 LDS");
  const int t = threadIdx.x, k = a.k, S = a.S;
  const long d = blockIdx.x, kk = (long)k * k;
  const bool ex = a.mode == GD_EXP;
  double* Z1 = a.Z1a + d * kk;
  double* Z2a = a.Z2a + d * kk;
  double* Z2b = a.Z2b + d * kk;
  double* al = a.alpha + d * S * k;
  double* be = a.beta + d * S * k;
  float* spec = a.spec + d * k;
  const int degenerate = a.fa[d * a.fa_stride] != 0 || (!ex && a.fb[d] != 0);
  if (degenerate) {                                // (uniform) NaN coefficients: every output of the pair is NaN
    for (int e = t; e < k * k; e += NT) { Z1[e] = nan64(); Z2b[e] = nan64(); if (ex) Z2a[e] = nan64(); }
    for (int e = t; e < S * k; e += NT) { al[e] = nan64(); be[e] = nan64(); }
    for (int e = t; e < k; e += NT) spec[e] = (float)nan64();
    if (t == 0) a.flags[d] = 1;
    return;
  }
  const double* Wa = a.Wa + d * a.wa_stride;
  const double* Wb = ex ? Wa : a.Wb + d * kk;      // the right-hand whitening of the k x k product below
  const double* Gab = a.Gab + d * kk;
  // Mm = Wa X Wb^T, X = A B^T (pair) or (P H^T)^T (exp)
  for (int e = t; e < k * k; e += NT) A[e / k][e % k] = ex ? Gab[(e % k) * k + e / k] : Gab[e];
  __syncthreads();
  for (int e = t; e < k * k; e += NT) {            // (Wa lower triangular)
    const int r = e / k, c = e % k;
    double s = 0.0;
    for (int b = 0; b <= r; ++b) s += Wa[r * k + b] * A[b][c];
    V[r][c] = s;
  }
  __syncthreads();
  for (int e = t; e < k * k; e += NT) {
    const int r = e / k, c = e % k;
    double s = 0.0;
    for (int b = 0; b <= c; ++b) s += V[r][b] * Wb[c * k + b];
    Mm[r][c] = s;
  }
  __syncthreads();
  if (ex) {                                        // V = W (H H^T), for the first term of S below
    const double* Ghh = a.Wb + d * kk;
    for (int e = t; e < k * k; e += NT) A[e / k][e % k] = Ghh[(e / k <= e % k) ? e : (e % k) * k + e / k];      // the upper half, mirrored
    __syncthreads();
    for (int e = t; e < k * k; e += NT) {
      const int r = e / k, c = e % k;
      double s = 0.0;
      for (int b = 0; b <= r; ++b) s += Wa[r * k + b] * A[b][c];
      V[r][c] = s;
    }
    __syncthreads();
  }
  for (int e = t; e < k * k; e += NT) {            // S = I - M M^T (pair), W (H H^T) W^T - K K^T (exp); the upper half mirrored
    const int r = e / k, c = e % k;
    if (r <= c) {
      double s = 0.0, g = r == c ? 1.0 : 0.0;
      for (int b = 0; b < k; ++b) s += Mm[r][b] * Mm[c][b];
      if (ex) {
        g = 0.0;
        for (int b = 0; b <= c; ++b) g += V[r][b] * Wa[c * k + b];
      }
      const double v = g - s;
      A[r][c] = v; A[c][r] = v;
    }
  }
  __syncthreads();
  jacobi_lds<KMAX, NT>(A, V, ws, k);
  if (t < k) {
    const double l = A[t][t];
    lam[t] = l < 0.0 ? 0.0 : ((!ex && l > 1.0) ? 1.0 : l);      // (a NaN stays a NaN)
  }
  __syncthreads();
  for (int e = t; e < k * k; e += NT) {            // U = V^T Mm into A (its diagonal has been read)
    const int r = e / k, c = e % k;
    double s = 0.0;
    for (int b = 0; b < k; ++b) s += V[b][r] * Mm[b][c];
    A[r][c] = s;
  }
  __syncthreads();
  if (t < k) {
    const double l = lam[t];
    if (ex) {
      val[t] = sqrt(l);                            // sigma
    } else {
      // small angles take the sine from the eigenvalue of S, large ones the cosine from ||U_t||^2 (fr_basis_kernel)
      double sn, cs, th;
      if (l <= 0.5) {
        sn = sqrt(l); cs = sqrt(1.0 - l); th = asin(sn);
      } else {
        double c2 = 0.0;
        for (int b = 0; b < k; ++b) c2 += A[t][b] * A[t][b];
        c2 = c2 > 1.0 ? 1.0 : c2;
        cs = sqrt(c2); sn = sqrt(1.0 - c2); th = acos(cs);
      }
      val[t] = th; csv[t] = cs; snv[t] = sn;
    }
    int best = 0;                                  // the sign of eigenvector t: its entry of largest magnitude, lowest index on ties, is positive
    double big = fabs(V[0][t]);
    for (int c = 1; c < k; ++c) {
      const double m = fabs(V[c][t]);
      if (m > big) { big = m; best = c; }
    }
    sgn[t] = V[best][t] < 0.0 ? -1.0 : 1.0;
  }
  __syncthreads();
  if (t < k) ord[rank_desc(val, k, t)] = t;  // descending; ties by index (rank counting)
  __syncthreads();
  const bool refused = !ex && val[ord[0]] > GD_DOMAIN;         // (uniform)
  if (refused) {
    for (int e = t; e < k * k; e += NT) { Z1[e] = nan64(); Z2b[e] = nan64(); }
    for (int e = t; e < S * k; e += NT) { al[e] = nan64(); be[e] = nan64(); }
    for (int e = t; e < k; e += NT) spec[e] = (float)nan64();
    if (t == 0) a.flags[d] = 2;
    return;
  }
  for (int e = t; e < k; e += NT) spec[e] = (float)val[ord[e]];
  if (t == 0) a.flags[d] = 0;
  for (int e = t; e < k * k; e += NT) {            // element [source row b][output row i]
    const int b = e / k, i = e % k, x = ord[i];
    double s = 0.0, u = 0.0;
    for (int c = b; c < k; ++c) { s += V[c][x] * Wa[c * k + b]; u += A[x][c] * Wb[c * k + b]; }
    Z1[e] = sgn[x] * s;                            // (V^T Wa)
    if (ex) { Z2a[e] = -sgn[x] * u; Z2b[e] = sgn[x] * s; }      // -(V^T K W) on P, (V^T W) on H
    else Z2b[e] = sgn[x] * u / csv[x];             // diag(1 / cos theta) U Wb
  }
  for (int e = t; e < S * k; e += NT) {
    const int j = e / k, x = ord[e % k];
    const double tt = a.ts.t[j], v = val[x];
    double p, q;
    if (ex) {
      p = cos(tt * v);
      q = v > 0.0 ? sin(tt * v) / v : tt;
    } else if (a.mode == GD_GEODESIC) {
      const double sn = snv[x];
      p = sn > 0.0 ? sin((1.0 - tt) * v) / sn : 1.0 - tt;
      q = sn > 0.0 ? sin(tt * v) / sn : tt;
    } else if (a.mode == GD_LOG && j == 1) {
      const double sn = snv[x];
      p = sn > 0.0 ? -v * csv[x] / sn : -1.0;
      q = sn > 0.0 ? v / sn : 1.0;
    } else {                                       // slice 0: pa; slice 1 of GD_VECTORS: pb
      p = j == 0 ? 1.0 : 0.0;
      q = j == 0 ? 0.0 : 1.0;
    }
    al[e] = p; be[e] = q;
  }
}

// Output slice s of pair d, rows i: alpha[d][s][i] (Z1a X)_i + beta[d][s][i] (Z2a X + Z2b Y)_i, X = Xs + d xstride, Y = Ys + d k N; one pass over the 2k
// rows.  Lane and column ownership of fr_stream_kernel: a wave owns 64 columns, lane (j = l & 15, g = l >> 4) loads the columns 4j .. 4j+3 of row r0 + g
// in one 16-byte access and feeds column e to the MFMAs of tile e; C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 * reg.  Both tiles stay in
// registers (2 KT 4 double4 accumulators).  EXP: the second tile also takes rows of X (Z2a).  vec: 16-byte accesses are legal.
// Slices: split = 0: slice s at O0 + (d S + s) k N; split = 1 (S = 2): slice 0 at O0 + d k N, slice 1 at O1 + d k N.
template <int KT, bool EXP>
__global__ __launch_bounds__(256) void gd_stream_kernel(const float* Xs, long xstride, const float* Ys, const double* Z1a, const double* Z2a,
                                                        const double* Z2b, const double* alpha, const double* beta, float* O0, float* O1, int split, int S,
                                                        int k, long N, int vec) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const long d = blockIdx.y;
  const long n0 = ((long)blockIdx.x * 4 + wave) * 64 + 4 * j;       // this lane's first column
  if (((long)blockIdx.x * 4 + wave) * 64 >= N) return;               // wave-uniform (no workgroup barrier in this kernel)
  const float* X = Xs + d * xstride;
  const float* Y = Ys + d * k * N;
  const double* z1a = Z1a + d * k * k;
  const double* z2a = Z2a + d * k * k;
  const double* z2b = Z2b + d * k * k;
  geom_d4 acc1[KT][4], acc2[KT][4];
#pragma unroll
  for (int m = 0; m < KT; ++m)
#pragma unroll
    for (int e = 0; e < 4; ++e) { acc1[m][e] = geom_d4{0.0, 0.0, 0.0, 0.0}; acc2[m][e] = geom_d4{0.0, 0.0, 0.0, 0.0}; }
  for (int r0 = 0; r0 < k; r0 += 4) {              // the rows of X
    const int r = r0 + g;
    const float4 x = r < k ? load4(X + (long)r * N, n0, N, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
    mfma_rows4<KT>(acc1, z1a, r, r < k, j, k, x);
    if (EXP) mfma_rows4<KT>(acc2, z2a, r, r < k, j, k, x);           // the one loaded x feeds both tiles
  }
  for (int r0 = 0; r0 < k; r0 += 4) {              // the rows of Y
    const int r = r0 + g;
    const float4 x = r < k ? load4(Y + (long)r * N, n0, N, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
    mfma_rows4<KT>(acc2, z2b, r, r < k, j, k, x);
  }
  if (n0 >= N) return;
  for (int s = 0; s < S; ++s) {
    const double* al = alpha + (d * S + s) * k;
    const double* be = beta + (d * S + s) * k;
    float* O = split ? (s == 0 ? O0 : O1) + d * k * N : O0 + (d * S + s) * k * N;
#pragma unroll
    for (int m = 0; m < KT; ++m)
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int i = 16 * m + g + 4 * x;
        if (i >= k) continue;
        const double p = al[i], q = be[i];
        store4(O + (long)i * N, n0, N, vec,
               make_float4((float)fma(q, acc2[m][0][x], p * acc1[m][0][x]), (float)fma(q, acc2[m][1][x], p * acc1[m][1][x]),
                           (float)fma(q, acc2[m][2][x], p * acc1[m][2][x]), (float)fma(q, acc2[m][3][x], p * acc1[m][3][x])));
      }
  }
}

// ------------------------------------------------------------------------------------------------------------ host side
namespace {
struct GdLayout { size_t big = 0, wa = 0, wb = 0, gab = 0, flags = 0, z1a = 0, z2a = 0, z2b = 0, alpha = 0, beta = 0, total = 0; long chunk = 0; };
bool gd_layout(long D, int S, int k, long N, GdLayout& l) {
  if (D < 1 || D > GD_MAX_PAIRS || S < 1 || S > GD_MAX_SLICES || k < 1 || k > FRECHET_MAX_RANK || N < 1 || k > N) return false;
  ScratchCarver s;
  const size_t kk = (size_t)k * k * sizeof(double), Sx = S < 2 ? 2 : S;
  l.chunk = GD_CHUNK_ROWS / k < 1 ? 1 : GD_CHUNK_ROWS / k;         // pairs per stacked Gram call
  if (l.chunk > D) l.chunk = D;
  const size_t cr = (size_t)l.chunk * k;
  l.big = s.take(cr * cr * sizeof(double));
  l.wa = s.take((size_t)D * kk); l.wb = s.take((size_t)D * kk); l.gab = s.take((size_t)D * kk);
  l.flags = s.take(2 * (size_t)D * sizeof(int));
  l.z1a = s.take((size_t)D * kk); l.z2a = s.take((size_t)D * kk); l.z2b = s.take((size_t)D * kk);
  l.alpha = s.take((size_t)D * Sx * k * sizeof(double)); l.beta = s.take((size_t)D * Sx * k * sizeof(double));
  l.total = s.off;
  return true;
}

// X: the first source (A or P), xstride 0 (one for all pairs) or k N; Y: the second (B or H).  S slices (mode GD_VECTORS / GD_LOG: 2, split over O0, O1).
int gd_run(const char* who, const float* X, long xstride, const float* Y, long D, int k, long N, int mode, const double* ts, int J, float* O0, float* O1,
           float* spec, int* flags, void* scratch, size_t scratch_bytes, hipStream_t st) {
  const bool timed = mode == GD_GEODESIC || mode == GD_EXP;
  const int S = timed ? J : 2;
  GdLayout l;
  if (!gd_layout(D, S, k, N, l)) {
    set_error("%s: D=%ld outside [1,%d], J=%d outside [1,%d], k=%d outside [1,%d], or N=%ld < k", who, D, GD_MAX_PAIRS, S, GD_MAX_SLICES, k,
              FRECHET_MAX_RANK, N);
    return -1;
  }
  if (xstride != 0 && xstride != (long)k * N) { set_error("%s: a_stride=%ld must be 0 (one basis for all pairs) or k N = %ld", who, xstride, (long)k * N); return -1; }
  if (timed && !ts) { set_error("%s: ts is null", who); return -1; }
  if (check_scratch(who, scratch, scratch_bytes, l.total, "dpb_grassmann_scratch_bytes(%ld, %d, %d, %ld)", D, S, k, N) != 0) return -1;
  char* base = (char*)scratch;
  double* big = (double*)(base + l.big);
  double* Wa = (double*)(base + l.wa);
  double* Wb = (double*)(base + l.wb);
  double* Gab = (double*)(base + l.gab);
  int* fa = (int*)(base + l.flags);
  int* fb = fa + D;
  const long kk = (long)k * k, kN = (long)k * N;
  const dim3 t256(256);
  // the three k x k Gram blocks of every pair: stacked calls of at most GD_CHUNK_ROWS rows, the blocks on the diagonal kept
  if (!xstride && launch_cross_gram(X, nullptr, Wa, k, k, N, st) != 0) return -1;
  for (long c0 = 0; c0 < D; c0 += l.chunk) {
    const long c = c0 + l.chunk < D ? l.chunk : D - c0;
    const int cr = (int)(c * k);
    if (xstride) {
      if (launch_cross_gram(X + c0 * kN, nullptr, big, cr, cr, N, st) != 0) return -1;
      launch_gram_blocks(big, Wa + c0 * kk, (int)c, cr, k, k, st);
    }
    if (launch_cross_gram(Y + c0 * kN, nullptr, big, cr, cr, N, st) != 0) return -1;
    launch_gram_blocks(big, Wb + c0 * kk, (int)c, cr, k, k, st);
    if (launch_cross_gram(xstride ? X + c0 * kN : X, Y + c0 * kN, big, xstride ? cr : k, cr, N, st) != 0) return -1;
    launch_gram_blocks(big, Gab + c0 * kk, (int)c, cr, xstride ? k : 0, k, st);
  }
  launch_angles_prep(Wa, fa, xstride ? (int)D : 1, k, st);
  if (mode != GD_EXP) launch_angles_prep(Wb, fb, (int)D, k, st);
  GdPairArgs a;
  a.Wa = Wa; a.wa_stride = xstride ? kk : 0; a.Wb = Wb; a.Gab = Gab; a.fa = fa; a.fa_stride = xstride ? 1 : 0; a.fb = fb;
  a.Z1a = (double*)(base + l.z1a); a.Z2a = (double*)(base + l.z2a); a.Z2b = (double*)(base + l.z2b);
  a.alpha = (double*)(base + l.alpha); a.beta = (double*)(base + l.beta);
  a.spec = spec; a.flags = flags; a.S = S; a.k = k; a.mode = mode;
  for (int j = 0; j < GD_MAX_SLICES; ++j) a.ts.t[j] = (timed && j < J) ? ts[j] : 0.0;
  DPB_BY_RANK(k, DPB_LAUNCH((gd_pair_kernel<KM, NT>), dim3((unsigned)D), dim3(NT), 0, st, a));
  const int split = timed ? 0 : 1;
  const int vec = (N % 4 == 0 && (uintptr_t)X % 16 == 0 && (uintptr_t)Y % 16 == 0 && (uintptr_t)O0 % 16 == 0 && (!split || (uintptr_t)O1 % 16 == 0)) ? 1 : 0;
  const dim3 sg((unsigned)((N + 255) / 256), (unsigned)D);
  if (mode == GD_EXP)
    DPB_BY_TILES(k, DPB_LAUNCH((gd_stream_kernel<KT, true>), sg, t256, 0, st, X, xstride, Y, a.Z1a, a.Z2a, a.Z2b, a.alpha, a.beta, O0, O1, split, S, k, N, vec));
  else
    DPB_BY_TILES(k, DPB_LAUNCH((gd_stream_kernel<KT, false>), sg, t256, 0, st, X, xstride, Y, a.Z1a, a.Z2a, a.Z2b, a.alpha, a.beta, O0, O1, split, S, k, N, vec));
  DPB_CHECK(hipGetLastError());
  return 0;
}
}  // namespace

}  // namespace dpb

// ------------------------------------------------------------------------------------------------------------ C ABI (include/dpb.h)
extern "C" {

size_t dpb_grassmann_scratch_bytes(int D, int J, int k, int64_t N) {
  dpb::GdLayout l;
  return dpb::gd_layout(D, J, k, N, l) ? l.total : 0;
}

int dpb_grassmann_pair(const float* A, int64_t a_stride, const float* B, int D, int k, int64_t N, int mode, const double* ts, int J, float* out0,
                       float* out1, float* theta, int32_t* flags, void* scratch, size_t scratch_bytes, void* hip_stream) {
  if (mode < dpb::GD_VECTORS || mode > dpb::GD_GEODESIC) { dpb::set_error("dpb_grassmann_pair: mode=%d outside [0,2]", mode); return -1; }
  if (!A || !B || !out0 || (mode != dpb::GD_GEODESIC && !out1) || !theta || !flags || !scratch) { dpb::set_error("dpb_grassmann_pair: null argument"); return -1; }
  return dpb::gd_run("dpb_grassmann_pair", A, a_stride, B, D, k, N, mode, ts, J, out0, out1, theta, flags, scratch, scratch_bytes, (hipStream_t)hip_stream);
}

int dpb_grassmann_exp(const float* P, const float* H, int D, int k, int64_t N, const double* ts, int J, float* Y, float* sigma, int32_t* flags,
                      void* scratch, size_t scratch_bytes, void* hip_stream) {
  if (!P || !H || !Y || !sigma || !flags || !scratch) { dpb::set_error("dpb_grassmann_exp: null argument"); return -1; }
  return dpb::gd_run("dpb_grassmann_exp", P, (long)k * N, H, D, k, N, dpb::GD_EXP, ts, J, Y, nullptr, sigma, flags, scratch, scratch_bytes,
                     (hipStream_t)hip_stream);
}

}  // extern "C"
