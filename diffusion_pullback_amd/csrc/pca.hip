// Randomized low-rank PCA of an fp32 feature matrix H [N][D] (N samples, D features): torch.pca_lowrank(H, q, center=True, niter), i.e.
// torch._lowrank._svd_lowrank + get_approximate_basis (Halko et al. 2009, algorithms 4.4 and 5.1), as the reference's global_pca_zt calls it
// (src/utils/utils.py:1017).  The QR factorisations become dpb_orth (orth.hip: rows spanning the same space -- the range finder depends on the
// span only), the final svd(B) is dpb_orth of B as well.
//
// Two product kernels on the f32-input MFMA (v_mfma_f32_32x32x2_f32: exact fp32 operands, fp32 accumulation) cover every step in both
// orientations, each with the column mean m subtracted from H as it is loaded (the centred H is never written; subtracting before the product
// rather than (P 1) m^T after it keeps the cancellation of a large mean out of the fp32 sums):
//   (a) Y[q][D] = P[q][N] (H - 1 m^T)      reduction over the samples, in full inside one wave
//   (b) Z[q][N] = Q[q][D] (H - 1 m^T)^T    reduction over the features, split over D; the splits' partials added in split order
// Every reduction has a fixed order (no atomics): the result is bitwise reproducible run to run.  All offsets into H are 64-bit (H of the up3
// tap passes 4 GiB at N = 820).
#include "kernels.h"

namespace dpb {

typedef float pca_f32x16 __attribute__((ext_vector_type(16)));

constexpr int PCA_KS = 8;             // consecutive reduction indices per lane per loop trip (two lane halves: 16 per trip)

// m[d] = mean over the samples of H[n][d]: one thread per column, an fp64 sum in sample order
__global__ __launch_bounds__(256) void pca_mean_kernel(const float* __restrict__ H, long N, long D, float* __restrict__ m) {
  const long d = (long)blockIdx.x * 256 + threadIdx.x;
  if (d >= D) return;
  double s = 0.0;
#pragma unroll 8
  for (long n = 0; n < N; ++n) s += (double)H[n * D + d];
  m[d] = (float)(s / (double)N);
}

// (a) Y[i][d] = sum_n P(i, n) (H[n][d] - m[d]) with P(i, n) = P[i * psi + n * psn] (R^T of the first product is R read transposed).
// A wave owns 32 columns d and all ceil(q / 32) = QT row tiles.  MFMA 32x32x2 operands: lane l holds A[i = l & 31][k = l >> 5] and
// B[k = l >> 5][j = l & 31]; a trip covers n0 .. n0 + 15, lane half h takes n0 + 8h + s at step s, for A and B alike.
template <int QT>
__global__ __launch_bounds__(256) void pca_prod_samples_kernel(const float* __restrict__ H, const float* __restrict__ m, const float* __restrict__ P,
                                                               long psi, long psn, float* __restrict__ Y, int q, long N, long D) {
  const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
  const long d0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
  if (d0 >= D) return;                                    // wave-uniform; no barrier in this kernel
  const long d = d0 + c;
  const bool dok = d < D;
  const float md = dok ? m[d] : 0.f;
  float a[QT][PCA_KS], b[PCA_KS];
  auto load = [&](long n0) {
#pragma unroll
    for (int s = 0; s < PCA_KS; ++s) {
      const long n = n0 + PCA_KS * h + s;
      const bool nok = n < N;
      b[s] = (nok && dok) ? H[n * D + d] - md : 0.f;
#pragma unroll
      for (int rt = 0; rt < QT; ++rt) {
        const int i = rt * 32 + c;
        a[rt][s] = (nok && i < q) ? P[i * psi + n * psn] : 0.f;
      }
    }
  };
  pca_f32x16 acc[QT];
#pragma unroll
  for (int rt = 0; rt < QT; ++rt) acc[rt] = pca_f32x16{};
  load(0);
  for (long n0 = 0; n0 < N; n0 += 2 * PCA_KS) {
    float ac[QT][PCA_KS], bc[PCA_KS];
#pragma unroll
    for (int s = 0; s < PCA_KS; ++s) {
      bc[s] = b[s];
#pragma unroll
      for (int rt = 0; rt < QT; ++rt) ac[rt][s] = a[rt][s];
    }
    load(n0 + 2 * PCA_KS);                                // next trip's operands in flight under this trip's MFMAs (guarded: zeros past N)
#pragma unroll
    for (int s = 0; s < PCA_KS; ++s)
#pragma unroll
      for (int rt = 0; rt < QT; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[rt][s], bc[s], acc[rt], 0, 0, 0);
  }
  if (!dok) return;
#pragma unroll
  for (int rt = 0; rt < QT; ++rt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {                        // C/D: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
      const int i = rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (i < q) Y[(long)i * D + d] = acc[rt][r];
    }
}

// (b) Zp[split][i][n] = sum_{d in split} Q(i, d) (H[n][d] - m[d]) with Q(i, d) = Q[i * qsi + d * qsd].  A wave owns 32 samples n (the B
// operand's columns) and all QT row tiles; a lane reads PCA_KS consecutive floats of its sample's row per trip.
template <int QT>
__global__ __launch_bounds__(256) void pca_prod_features_kernel(const float* __restrict__ H, const float* __restrict__ m, const float* __restrict__ Q,
                                                                long qsi, long qsd, float* __restrict__ Zp, int q, long N, long D, long dchunk) {
  const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
  const long n0w = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
  if (n0w >= N) return;                                   // wave-uniform
  const long n = n0w + c;
  const bool nok = n < N;
  const float* Hn = H + (nok ? n : 0) * D;
  const long dbeg = (long)blockIdx.y * dchunk, dend = dbeg + dchunk < D ? dbeg + dchunk : D;
  float a[QT][PCA_KS], b[PCA_KS];
  auto load = [&](long d0) {
#pragma unroll
    for (int s = 0; s < PCA_KS; ++s) {
      const long d = d0 + PCA_KS * h + s;
      const bool ok = d < dend;
      b[s] = (ok && nok) ? Hn[d] - m[d] : 0.f;
#pragma unroll
      for (int rt = 0; rt < QT; ++rt) {
        const int i = rt * 32 + c;
        a[rt][s] = (ok && i < q) ? Q[i * qsi + d * qsd] : 0.f;
      }
    }
  };
  pca_f32x16 acc[QT];
#pragma unroll
  for (int rt = 0; rt < QT; ++rt) acc[rt] = pca_f32x16{};
  load(dbeg);
  for (long d0 = dbeg; d0 < dend; d0 += 2 * PCA_KS) {
    float ac[QT][PCA_KS], bc[PCA_KS];
#pragma unroll
    for (int s = 0; s < PCA_KS; ++s) {
      bc[s] = b[s];
#pragma unroll
      for (int rt = 0; rt < QT; ++rt) ac[rt][s] = a[rt][s];
    }
    load(d0 + 2 * PCA_KS);
#pragma unroll
    for (int s = 0; s < PCA_KS; ++s)
#pragma unroll
      for (int rt = 0; rt < QT; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[rt][s], bc[s], acc[rt], 0, 0, 0);
  }
  if (!nok) return;
  float* Zs = Zp + (long)blockIdx.y * q * N;
#pragma unroll
  for (int rt = 0; rt < QT; ++rt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (i < q) Zs[(long)i * N + n] = acc[rt][r];
    }
}

// Z[e] = sum over the splits of Zp[split][e], in split order, fp64
__global__ __launch_bounds__(256) void pca_split_sum_kernel(const float* __restrict__ Zp, int nsplit, long qn, float* __restrict__ Z) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= qn) return;
  double s = 0.0;
  for (int sp = 0; sp < nsplit; ++sp) s += (double)Zp[(long)sp * qn + e];
  Z[e] = (float)s;
}

// svd(B) from the mixing matrix of dpb_orth(B): Cm = diag(sgn / sigma) E^T with E the Gram eigenvectors (B B^T = E diag(sigma^2) E^T), so row i
// of Cm has norm 1 / sigma_i.  Writes S = sigma (torch.linalg.svd's S of B) and Ub^T = diag(sigma) Cm (the left singular vectors, as rows; the
// signs pair them with the rows dpb_orth returned).  A zero row (sigma below orth's 1e-150 floor) gives S = 0 and a zero row of Ub^T.
__global__ void pca_svd_finish_kernel(const double* __restrict__ Cm, int q, float* __restrict__ S, double* __restrict__ UbT) {
  const int i = threadIdx.x;
  if (i >= q) return;
  double n2 = 0.0;
  for (int j = 0; j < q; ++j) n2 += Cm[i * q + j] * Cm[i * q + j];
  const double inv = !(n2 <= 0.0) ? 1.0 / sqrt(n2) : 0.0;   // = sigma_i (NaN for the NaN row dpb_orth leaves on non-finite input: S is NaN, not 0)
  S[i] = (float)inv;
  for (int j = 0; j < q; ++j) UbT[i * q + j] = Cm[i * q + j] * inv;
}

// u[i][d] = sum_j C[i][j] X[j][d] (fp64 sums): U = Q Ub of _svd_lowrank, rows.  The shape of orth_apply_tiled_kernel: one column per thread,
// the rows in tiles of 16, C of the tile in LDS.
__global__ __launch_bounds__(256) void pca_rotate_kernel(const double* __restrict__ C, const float* __restrict__ X, float* __restrict__ u, int q, long D) {
  constexpr int IT = 16;
  __shared__ double ct[IT * ORTH_MAX_RANK];
  for (int i0 = 0; i0 < q; i0 += IT) {
    __syncthreads();
    for (int e = threadIdx.x; e < IT * q; e += 256) ct[e] = i0 + e / q < q ? C[(long)i0 * q + e] : 0.0;
    __syncthreads();
    for (long d = (long)blockIdx.x * 256 + threadIdx.x; d < D; d += (long)gridDim.x * 256) {
      double v[IT];
#pragma unroll
      for (int i = 0; i < IT; ++i) v[i] = 0.0;
      for (int j = 0; j < q; ++j) {
        const double x = (double)X[(long)j * D + d];
#pragma unroll
        for (int i = 0; i < IT; ++i) v[i] += ct[i * q + j] * x;
      }
#pragma unroll
      for (int i = 0; i < IT; ++i)
        if (i0 + i < q) u[(long)(i0 + i) * D + d] = (float)v[i];
    }
  }
}

// ---------------------------------------------------------------- host side

// split of the feature reduction: enough blocks to fill the chip (about 2048 waves), at most 64 splits, at least 256 features per split
static void pca_split(long N, long D, int* nsplit, long* dchunk) {
  const long nbx = (N + 127) / 128;
  long s = (2048 / 4 + nbx - 1) / nbx;
  if (s > 64) s = 64;
  if (s > (D + 255) / 256) s = (D + 255) / 256;
  if (s < 1) s = 1;
  long ch = (D + s - 1) / s;
  ch = (ch + 2 * PCA_KS - 1) / (2 * PCA_KS) * (2 * PCA_KS);
  *dchunk = ch;
  *nsplit = (int)((D + ch - 1) / ch);
}

struct PcaLayout { size_t orth, ubt, m, wd, qd, wn, qn, zp, s, conv, total; };

static PcaLayout pca_layout(int q, long N, long D) {
  int ns; long ch;
  pca_split(N, D, &ns, &ch);
  PcaLayout L{};
  ScratchCarver c;
  const size_t ob_d = orth_scratch_bytes(q, D), ob_n = orth_scratch_bytes(q, N);
  L.orth = c.take(ob_d > ob_n ? ob_d : ob_n);
  L.ubt = c.take(sizeof(double) * q * q);
  L.m = c.take(sizeof(float) * D);
  L.wd = c.take(sizeof(float) * q * D);
  L.qd = c.take(sizeof(float) * q * D);
  L.wn = c.take(sizeof(float) * q * N);
  L.qn = c.take(sizeof(float) * q * N);
  L.zp = c.take(sizeof(float) * (size_t)ns * q * N);
  L.s = c.take(sizeof(float) * q);
  L.conv = c.take(sizeof(float) * 2);
  L.total = c.off + 256;                                      // + the caller's base alignment
  return L;
}

const char* pca_invalid(int q, long N, long D) {
  if (N < 2 || D < 1) return "H must have at least 2 samples and 1 feature";
  if (q < 1 || q > ORTH_MAX_RANK) return "q outside [1, 128] (the rank limit of the re-orthonormalisation)";
  if (q > N - 1) return "q > N - 1 (the centred H has rank at most N - 1)";
  if (q > D) return "q > D";
  return nullptr;
}

size_t pca_scratch_bytes(int q, long N, long D) { return pca_invalid(q, N, D) ? 0 : pca_layout(q, N, D).total; }

template <int QT>
static void prod_samples(const float* H, const float* m, const float* P, long psi, long psn, float* Y, int q, long N, long D, hipStream_t st) {
  DPB_LAUNCH((pca_prod_samples_kernel<QT>), dim3((unsigned)((D + 127) / 128)), dim3(256), 0, st, H, m, P, psi, psn, Y, q, N, D);
}
template <int QT>
static void prod_features(const float* H, const float* m, const float* Q, long qsi, long qsd, float* Zp, int q, long N, long D, long ch, int ns,
                          hipStream_t st) {
  DPB_LAUNCH((pca_prod_features_kernel<QT>), dim3((unsigned)((N + 127) / 128), ns), dim3(256), 0, st, H, m, Q, qsi, qsd, Zp, q, N, D, ch);
}

int launch_pca_lowrank(const float* H, long N, long D, const float* R, int q, int niter, float* u, float* s, void* scratch, size_t scratch_bytes,
                       hipStream_t st) {
  if (const char* why = pca_invalid(q, N, D)) { set_error("dpb_pca_lowrank: %s (q=%d, N=%ld, D=%ld)", why, q, N, D); return -1; }
  if (niter < 0) { set_error("dpb_pca_lowrank: niter=%d < 0", niter); return -1; }
  const PcaLayout L = pca_layout(q, N, D);
  if (scratch_bytes < L.total) { set_error("dpb_pca_lowrank: scratch of %zu bytes, dpb_pca_scratch_bytes(%d, %ld, %ld) = %zu", scratch_bytes, q, N, D, L.total); return -1; }
  char* base = (char*)scratch + ((256 - ((uintptr_t)scratch & 255)) & 255);
  double* orth_s = (double*)(base + L.orth);
  double* ubt = (double*)(base + L.ubt);
  float *m = (float*)(base + L.m), *Wd = (float*)(base + L.wd), *Qd = (float*)(base + L.qd), *Wn = (float*)(base + L.wn), *Qn = (float*)(base + L.qn);
  float *Zp = (float*)(base + L.zp), *s_orth = (float*)(base + L.s), *conv = (float*)(base + L.conv);
  int ns; long ch;
  pca_split(N, D, &ns, &ch);
  const int qt = (q + 31) / 32;

  // Y[q][D] = P (H - 1 m^T);  Z[q][N] = Q (H - 1 m^T)^T;  orthonormal rows of W's span (the QR of get_approximate_basis)
  auto prodA = [&](const float* P, long psi, long psn, float* Y) {
    switch (qt) {
      case 1: prod_samples<1>(H, m, P, psi, psn, Y, q, N, D, st); break;
      case 2: prod_samples<2>(H, m, P, psi, psn, Y, q, N, D, st); break;
      case 3: prod_samples<3>(H, m, P, psi, psn, Y, q, N, D, st); break;
      default: prod_samples<4>(H, m, P, psi, psn, Y, q, N, D, st); break;
    }
  };
  auto prodB = [&](const float* Q, long qsi, long qsd, float* Z) {
    switch (qt) {
      case 1: prod_features<1>(H, m, Q, qsi, qsd, Zp, q, N, D, ch, ns, st); break;
      case 2: prod_features<2>(H, m, Q, qsi, qsd, Zp, q, N, D, ch, ns, st); break;
      case 3: prod_features<3>(H, m, Q, qsi, qsd, Zp, q, N, D, ch, ns, st); break;
      default: prod_features<4>(H, m, Q, qsi, qsd, Zp, q, N, D, ch, ns, st); break;
    }
    const long qn = (long)q * N;
    DPB_LAUNCH(pca_split_sum_kernel, dim3((unsigned)((qn + 255) / 256)), dim3(256), 0, st, Zp, ns, qn, Z);
  };
  auto orth = [&](const float* W, float* V, long len) -> int {
    OrthArgs a;                                           // Vprev = W: the rows are signed to overlap W's (any sign spans the same space)
    a.W = W; a.Vprev = W; a.V = V; a.s = s_orth; a.conv = conv; a.scratch = orth_s; a.k = q; a.N = len;
    a.scratch_bytes = orth_scratch_bytes(q, len);
    return launch_orth(a, st);
  };

  DPB_LAUNCH(pca_mean_kernel, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, st, H, N, D, m);
  if (N < D) {
    // _svd_lowrank transposes: A = Hc^T [D][N], R [N][q].  Basis rows Qd [q][D] (Q^T of get_approximate_basis).
    prodA(R, 1, q, Wd);                                   // X = A R          -> X^T = R^T Hc
    if (int r = orth(Wd, Qd, D)) return r;
    for (int it = 0; it < niter; ++it) {
      prodB(Qd, D, 1, Wn);                                // X = A^H Q = Hc Q  -> [q][N]
      if (int r = orth(Wn, Qn, N)) return r;
      prodA(Qn, N, 1, Wd);                                // X = A Q = Hc^T Q  -> [q][D]
      if (int r = orth(Wd, Qd, D)) return r;
    }
    prodB(Qd, D, 1, Wn);                                  // B = Q^H A = Q^T Hc^T [q][N]
    if (int r = orth(Wn, Qn, N)) return r;                // svd(B): Vb rows (unused), mixing matrix in orth_s
    DPB_LAUNCH(pca_svd_finish_kernel, dim3(1), dim3(ORTH_MAX_RANK), 0, st, orth_s, q, s, ubt);
    // after the swap the reference's u (_svd_lowrank's V) is Q Ub [D][q]: rows Ub^T Qd
    DPB_LAUNCH(pca_rotate_kernel, dim3((unsigned)((D + 255) / 256 < 1024 ? (D + 255) / 256 : 1024)), dim3(256), 0, st, ubt, Qd, u, q, D);
  } else {
    // A = Hc [N][D], R [D][q].  Basis rows Qn [q][N].
    prodB(R, 1, q, Wn);                                   // X = A R = Hc R    -> [q][N]
    if (int r = orth(Wn, Qn, N)) return r;
    for (int it = 0; it < niter; ++it) {
      prodA(Qn, N, 1, Wd);                                // X = A^H Q = Hc^T Q -> [q][D]
      if (int r = orth(Wd, Qd, D)) return r;
      prodB(Qd, D, 1, Wn);                                // X = A Q = Hc Q     -> [q][N]
      if (int r = orth(Wn, Qn, N)) return r;
    }
    prodA(Qn, N, 1, Wd);                                  // B = Q^H A [q][D]
    if (int r = orth(Wd, u, D)) return r;                 // svd(B): its right singular vectors (rows) are the reference's u, as rows
    DPB_LAUNCH(pca_svd_finish_kernel, dim3(1), dim3(ORTH_MAX_RANK), 0, st, orth_s, q, s, ubt);
  }
  DPB_CHECK(hipGetLastError());
  return 0;
}

}  // namespace dpb
