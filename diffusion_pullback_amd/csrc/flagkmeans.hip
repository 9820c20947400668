// Flag k-means: Lloyd's algorithm on the Grassmannian with rank-r flag means as centres and r - a as the distance, a(A, Y) = sum_j cos^2 theta_j(A, Y) =
// ||Q_Y Q_A^T||_F^2 the chordal affinity of two subspaces of any two ranks; and that affinity between two stacks (dpb_flag_affinity).
//
// The rank-r flag mean of a cluster is the r-dimensional subspace that maximises the summed affinity of its members, so refitting the centres cannot
// raise J = sum_i (r - a[i, label_i]) and neither can moving a member to the centre it holds best: the argument of ordinary k-means.
//
// Everything between the two passes over the rows (the Gram before, the centres after) runs on coefficients against the whitened fp64 Gram
// Ghat = Q Q^T [R][R] of all R = B k rows (launch_whitened_gram, frechet.hip), Q_i = W_i X_i the orthonormalised members:
//   seeding  D^2(i, s) = k - ||Ghat_is||_F^2 per block column of a seed (fk_seed_dist_kernel); farthest-first picks on the device (fk_seed_pick_kernel)
//   update   Ghat[I_c, I_c], members ascending, gathered into a contiguous matrix (fk_gather_kernel); the flag-mean solver of flagmean.hip runs on it
//            as on any caller's Ghat and returns Ct_c [R_c][r], Y_c = Ct_c^T Q[I_c], Ct_c^T Ghat_cc Ct_c = I; fk_scatter_kernel files the rows of Ct_c
//            under their members' rows of Z [R][r]
//   assign   S[:, c-block] = sum_{j in c} Ghat[:, j-block] Z[j-rows] = Q Y_c^T for every cluster in ONE pass over Ghat (fk_product_kernel, on
//            v_mfma_f64_16x16x4_f64: 2 R^2 r flops); a[i, c] = ||S[i-rows, c-block]||_F^2 and the member's wish (fk_affinity_kernel); the objective,
//            the keep-the-last-member rule, the new labels and the new member lists (fk_move_kernel)
//   finish   the coefficients on the rows as given, Z blockdiag(W) (fk_coef_kernel), and launch_coef_stream
// Reproducibility: fp64, no atomics, every sum a fixed chain -- the reduction range of the product is cut among the waves of a workgroup at bounds
// that depend on the member list only and the partial tiles are added in wave order.
#include "kernels.h"
#include "geom.h"

namespace dpb {

// ------------------------------------------------------------------------------------------------------------ the affinity of two stacks
// Workgroups walk the pairs p = blockIdx.x, blockIdx.x + gridDim.x, ...; pair (i, c) = (p / Bc, p % Bc).  T = W_i G_ic [k][r] (W_i lower triangular),
// M = T W'_c^T, aff = sum M^2: every element a sequential sum, the squares added by block_sum -- a function of the pair's blocks alone
__global__ __launch_bounds__(256) void fk_pair_affinity_kernel(const double* Wa, const double* Wb, const int* fa, const int* fb, const double* Gab, long ldg,
                                                               double* aff, int Ba, int Bc, int k, int r) {
  __shared__ double Gl[64][65], Tl[64][65], red[4];
  const int t = threadIdx.x;
  for (long p = blockIdx.x; p < (long)Ba * Bc; p += gridDim.x) {
    const int i = (int)(p / Bc), c = (int)(p % Bc);
    if (fa[i] != 0 || fb[c] != 0) {                  // NaN for a degenerate basis's row and column
      if (t == 0) aff[p] = nan64();
      continue;
    }
    const double* Wi = Wa + (long)i * k * k;
    const double* Wc = Wb + (long)c * r * r;
    const double* Gic = Gab + (long)i * k * ldg + (long)c * r;
    __syncthreads();                                 // the previous pair is done with the LDS
    for (int e = t; e < k * r; e += 256) Gl[e / r][e % r] = Gic[(long)(e / r) * ldg + e % r];
    __syncthreads();
    for (int e = t; e < k * r; e += 256) {
      const int a = e / r, b = e % r;
      double s = 0.0;
      for (int x = 0; x <= a; ++x) s += Wi[a * k + x] * Gl[x][b];
      Tl[a][b] = s;
    }
    __syncthreads();
    double sq = 0.0;
    for (int e = t; e < k * r; e += 256) {
      const int a = e / r, b = e % r;
      double s = 0.0;
      for (int x = 0; x <= b; ++x) s += Tl[a][x] * Wc[b * r + x];
      sq += s * s;
    }
    const double tot = block_sum<256>(sq, red);
    if (t == 0) aff[p] = tot;
  }
}

constexpr long FK_PAIR_BLOCKS = 4096;

namespace {
struct FaLayout { size_t gab = 0, wa = 0, wb = 0, flags = 0, total = 0; };
bool fa_layout(long Ba, int k, long Bc, int r, long N, FaLayout& l) {
  if (Ba < 1 || Bc < 1 || Ba > 65535 || Bc > 65535 || k < 1 || k > FLAG_MEAN_MAX_RANK || r < 1 || r > FLAG_MEAN_MAX_RANK || N < 1 || k > N || r > N) return false;
  ScratchCarver s;
  l.gab = s.take((size_t)Ba * k * (size_t)Bc * r * sizeof(double));
  l.wa = s.take((size_t)Ba * k * k * sizeof(double));
  l.wb = s.take((size_t)Bc * r * r * sizeof(double));
  l.flags = s.take((size_t)(Ba + Bc) * sizeof(int));
  l.total = s.off;
  return true;
}
}  // namespace

size_t flag_affinity_scratch_bytes(long Ba, int k, long Bc, int r, long N) {
  FaLayout l;
  return fa_layout(Ba, k, Bc, r, N, l) ? l.total : 0;
}

int launch_flag_affinity(const float* A, const float* Y, long Ba, int k, long Bc, int r, long N, double* aff, void* scratch, size_t scratch_bytes,
                         hipStream_t st) {
  FaLayout l;
  if (!fa_layout(Ba, k, Bc, r, N, l)) {
    set_error("dpb_flag_affinity: B=%ld, C=%ld outside [1,65535], k=%d or r=%d outside [1,%d], or N=%ld < max(k, r)", Ba, Bc, k, r, FLAG_MEAN_MAX_RANK, N);
    return -1;
  }
  if (check_scratch("dpb_flag_affinity", scratch, scratch_bytes, l.total, "dpb_flag_affinity_scratch_bytes(%ld, %d, %ld, %d, %ld)", Ba, k, Bc, r, N) != 0)
    return -1;
  char* base = (char*)scratch;
  double* Gab = (double*)(base + l.gab);
  double* Wa = (double*)(base + l.wa);
  double* Wb = (double*)(base + l.wb);
  int* fa = (int*)(base + l.flags);
  int* fb = fa + Ba;
  const int Ra = (int)(Ba * k), Rb = (int)(Bc * r);
  if (launch_cross_gram(A, Y, Gab, Ra, Rb, N, st) != 0) return -1;
  if (launch_self_gram_blocks(A, Wa, (int)Ba, k, N, st) != 0 || launch_self_gram_blocks(Y, Wb, (int)Bc, r, N, st) != 0) return -1;
  launch_angles_prep(Wa, fa, (int)Ba, k, st);
  launch_angles_prep(Wb, fb, (int)Bc, r, st);
  const long pairs = Ba * Bc;
  DPB_LAUNCH(fk_pair_affinity_kernel, dim3((unsigned)(pairs < FK_PAIR_BLOCKS ? pairs : FK_PAIR_BLOCKS)), dim3(256), 0, st, Wa, Wb, fa, fb, Gab, (long)Rb, aff,
             (int)Ba, (int)Bc, k, r);
  DPB_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------------------------ k-means: the state
struct FkHead {           // the first 32 bytes of the scratch block (documented in dpb.h: the caller reads them, and the lists after them, once per round)
  int moved, kept, n_degenerate, pad;
  double J, pad1;
};

namespace {
struct FkLayout {
  size_t head = 0, sizes = 0, changed = 0, seeds = 0, labels = 0, flags = 0;        // the part the host reads: contiguous from 0
  size_t host_bytes = 0;
  size_t offs = 0, order = 0, want = 0, dmin = 0, aff = 0, W = 0, Z = 0, S = 0, G = 0, total = 0;
};
bool fk_layout(long B, int k, long N, long C, int r, FkLayout& l) {
  if (B < 1 || B > 65535 || k < 1 || k > FRECHET_MAX_RANK || B * k > (1 << 20) || N < 1 || k > N || C < 1 || C > B || r < 1 || r > k) return false;
  const size_t R = (size_t)B * k;
  size_t off = 0;                                       // the host part is packed (no rounding between its pieces)
  l.head = off; off += sizeof(FkHead);
  l.sizes = off; off += (size_t)C * sizeof(int);
  l.changed = off; off += (size_t)C * sizeof(int);
  l.seeds = off; off += (size_t)C * sizeof(int);
  l.labels = off; off += (size_t)B * sizeof(int);
  l.flags = off; off += (size_t)B * sizeof(int);
  l.host_bytes = off;
  ScratchCarver s;
  s.take(off);
  l.offs = s.take((size_t)(C + 1) * sizeof(int));
  l.order = s.take((size_t)B * sizeof(int));
  l.want = s.take((size_t)B * sizeof(int));
  l.dmin = s.take((size_t)B * sizeof(double));
  l.aff = s.take((size_t)B * C * sizeof(double));
  l.W = s.take((size_t)B * k * k * sizeof(double));
  l.Z = s.take(R * r * sizeof(double));
  l.S = s.take(R * (size_t)C * r * sizeof(double));
  l.G = s.take(R * R * sizeof(double));
  l.total = s.off;
  return true;
}
struct FkPtrs {
  FkHead* head; int *sizes, *changed, *seeds, *labels, *flags, *offs, *order, *want; double *dmin, *aff, *W, *Z, *S, *G;
};
FkPtrs fk_ptrs(void* scratch, const FkLayout& l) {
  char* b = (char*)scratch;
  FkPtrs p;
  p.head = (FkHead*)(b + l.head); p.sizes = (int*)(b + l.sizes); p.changed = (int*)(b + l.changed); p.seeds = (int*)(b + l.seeds);
  p.labels = (int*)(b + l.labels); p.flags = (int*)(b + l.flags); p.offs = (int*)(b + l.offs); p.order = (int*)(b + l.order); p.want = (int*)(b + l.want);
  p.dmin = (double*)(b + l.dmin); p.aff = (double*)(b + l.aff); p.W = (double*)(b + l.W); p.Z = (double*)(b + l.Z); p.S = (double*)(b + l.S);
  p.G = (double*)(b + l.G);
  return p;
}
int fk_check(const char* who, long B, int k, long N, long C, int r, const void* scratch, size_t scratch_bytes, FkLayout& l) {
  if (!fk_layout(B, k, N, C, r, l)) {
    set_error("%s: B=%ld outside [1,65535], k=%d outside [1,%d], N=%ld < k, B k above 2^20, C=%ld outside [1,B] or r=%d outside [1,k]", who, B, k,
              FRECHET_MAX_RANK, N, C, r);
    return -1;
  }
  return check_scratch(who, scratch, scratch_bytes, l.total, "dpb_flag_kmeans_scratch_bytes(%ld, %d, %ld, %ld, %d)", B, k, N, C, r);
}
}  // namespace

// ------------------------------------------------------------------------------------------------------------ seeding and the start labels
// block i: d = k - ||Ghat[i-block, s-block]||_F^2 for s = seeds[t], the t-th seed; dmin[i] and the nearest seed so far (labels[i]) follow, the lower
// cluster kept on a tie; a seed takes its own cluster and leaves the race (dmin = -1e300); a degenerate member: dmin NaN, label -1
__global__ __launch_bounds__(256) void fk_seed_dist_kernel(const double* G, const int* flags, const int* seeds, int t, double* dmin, int* labels, long R, int k) {
  __shared__ double red[4];
  const int i = blockIdx.x, s = seeds[t];
  if (flags[i] != 0) {
    if (threadIdx.x == 0) { dmin[i] = nan64(); labels[i] = -1; }
    return;
  }
  double sq = 0.0;
  for (int e = threadIdx.x; e < k * k; e += 256) {
    const double v = G[((long)i * k + e / k) * R + (long)s * k + e % k];
    sq += v * v;
  }
  const double d = (double)k - block_sum<256>(sq, red);
  if (threadIdx.x == 0) {
    if (i == s) { dmin[i] = -1e300; labels[i] = t; }
    else if (t == 0 || d < dmin[i]) { dmin[i] = d; labels[i] = t; }      // (a seed's dmin is -1e300: nothing is below it)
  }
}

// one workgroup: seeds[t + 1] = the member of largest dmin, the lowest index on a tie (degenerate members and seeds never win)
__global__ __launch_bounds__(256) void fk_seed_pick_kernel(const double* dmin, int* seeds, int t, int B) {
  __shared__ double bv[256];
  __shared__ int bi[256];
  const int th = threadIdx.x;
  double best = -2e300;
  int idx = -1;
  for (int i = th; i < B; i += 256) {
    const double v = dmin[i];
    if (v > best) { best = v; idx = i; }             // (a NaN compares false; a thread walks its members in index order)
  }
  bv[th] = best; bi[th] = idx;
  __syncthreads();
  if (th == 0) {
    double b = -2e300;
    int ix = -1;
    for (int e = 0; e < 256; ++e)
      if (bi[e] >= 0 && (bv[e] > b || (bv[e] == b && bi[e] < ix))) { b = bv[e]; ix = bi[e]; }
    seeds[t + 1] = ix < 0 ? 0 : ix;
  }
}

// one workgroup: the member lists of the labels -- sizes [C], offs [C + 1], order [B] in (label, index) order -- by a counting sort in index order;
// first: every cluster is marked changed and the head cleared
__global__ __launch_bounds__(256) void fk_lists_kernel(const int* labels, const int* flags, int* sizes, int* offs, int* order, int* changed, FkHead* head, int B,
                                                       int C, int first) {
  const int t = threadIdx.x;
  for (int c = t; c < C; c += 256) { sizes[c] = 0; if (first) changed[c] = 1; }
  __syncthreads();
  if (t == 0) {
    int nd = 0;
    for (int i = 0; i < B; ++i) { const int c = labels[i]; if (c >= 0) sizes[c] += 1; else nd += 1; }
    int o = 0;
    for (int c = 0; c < C; ++c) { offs[c] = o; o += sizes[c]; }
    offs[C] = o;
    if (first) { head->moved = 0; head->kept = 0; head->n_degenerate = nd; head->pad = 0; head->J = 0.0; head->pad1 = 0.0; }
    // every list filled in one scan in index order (sizes counts up again as the fill pointer)
    for (int c = 0; c < C; ++c) sizes[c] = 0;
    for (int i = 0; i < B; ++i) {
      const int c = labels[i];
      if (c >= 0) { order[offs[c] + sizes[c]] = i; sizes[c] += 1; }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ update: gather and scatter
// block (p, q): Gc[p-block][q-block] = Ghat[member p's rows][member q's rows], Gc [Rc][Rc] contiguous, the members of cluster c ascending
__global__ __launch_bounds__(256) void fk_gather_kernel(const double* G, const int* order, const int* offs, int c, int n_c, double* Gc, long R, int k) {
  if (offs[c + 1] - offs[c] != n_c) return;           // (the caller sized Gc and the grid for n_c members: anything else would leave its bounds)
  const int* mem = order + offs[c];
  const long Rc = (long)n_c * k;
  const long gi = (long)mem[blockIdx.y] * k, gj = (long)mem[blockIdx.x] * k;
  const long li = (long)blockIdx.y * k, lj = (long)blockIdx.x * k;
  for (int e = threadIdx.x; e < k * k; e += 256) Gc[(li + e / k) * Rc + lj + e % k] = G[(gi + e / k) * R + gj + e % k];
}

// block p: the rows of Ct_c [Rc][r] of member p of cluster c to that member's rows of Z [R][r]
__global__ __launch_bounds__(256) void fk_scatter_kernel(const double* Ct, const int* order, const int* offs, int c, int n_c, double* Z, int k, int r) {
  if (offs[c + 1] - offs[c] != n_c) return;
  const long src = (long)blockIdx.x * k * r, dst = (long)order[offs[c] + blockIdx.x] * k * r;
  for (int e = threadIdx.x; e < k * r; e += 256) Z[dst + e] = Ct[src + e];
}

// ------------------------------------------------------------------------------------------------------------ assignment: the pass over Ghat
// S[32 rows of the workgroup][c-block] = sum over the members j of cluster c = blockIdx.y of Ghat[rows][j-block] Z[j-rows][:r]: the workgroups of one
// row tile read every column of Ghat once between them, each column block against the coefficients of its own member's cluster only.  The reduction
// range of a workgroup is the cluster's list of (member, 16-column chunk) slots, ceil(k / 16) per member; its NW waves take an NW-th each, in list
// order, and their partial tiles are added in wave order.  Lane (j = l & 15, g = l >> 4) reads the four consecutive doubles
// Ghat[row j][member k + 16 cc + 4 g ..+3] of each 16-row tile -- one 32-byte access when k and R are multiples of 4 -- slots past the member's k
// columns carrying zeros, and feeds element e to MFMA e of the chunk; the B operand is Z[member k + 16 cc + 4 g + e][16 n + j].  The next chunk's
// operands are loaded before the current chunk's MFMAs issue.  C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 * reg.
template <int KT>
struct FkOperands {
  double a[2][4];
  double b[4][KT];
};

template <int KT>
__device__ __forceinline__ void fk_load(FkOperands<KT>& o, const double* __restrict__ G, const double* __restrict__ Z, const int* __restrict__ mem, int ch,
                                        int ch_hi, int cpm, int i0, int j, int g, int R, int k, int r, bool vec) {
  const bool live = ch < ch_hi;
  const int member = live ? mem[ch / cpm] : 0;
  const int cin = 16 * (ch % cpm) + 4 * g;             // the first of this lane's four columns inside the member's block
  const long col = (long)member * k + cin;
#pragma unroll
  for (int tl = 0; tl < 2; ++tl) {
    const int row = i0 + 16 * tl + j;
    const bool ok = live && row < R && cin < k;
    if (ok && vec) {                                    // (k % 4 == 0: cin + 3 < k)
      const geom_d4 v = *reinterpret_cast<const geom_d4*>(G + (long)row * R + col);
      o.a[tl][0] = v[0]; o.a[tl][1] = v[1]; o.a[tl][2] = v[2]; o.a[tl][3] = v[3];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) o.a[tl][e] = (ok && cin + e < k) ? G[(long)row * R + col + e] : 0.0;
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bool zok = live && cin + e < k;
#pragma unroll
    for (int n = 0; n < KT; ++n) o.b[e][n] = (zok && 16 * n + j < r) ? Z[(col + e) * r + 16 * n + j] : 0.0;
  }
}

template <int KT>
__device__ __forceinline__ void fk_mma(geom_d4 (&acc)[2][KT], const FkOperands<KT>& o) {
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int n = 0; n < KT; ++n) {
      acc[0][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(o.a[0][e], o.b[e][n], acc[0][n], 0, 0, 0);
      acc[1][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(o.a[1][e], o.b[e][n], acc[1][n], 0, 0, 0);
    }
}

template <int KT, int NW>
__global__ __launch_bounds__(NW * 64) void fk_product_kernel(const double* __restrict__ G, const double* __restrict__ Z, double* __restrict__ S,
                                                         const int* __restrict__ order, const int* __restrict__ offs, int R, int k, int r, int C) {
  __shared__ double red[NW][2][KT][4][64];
  static_assert(sizeof(double) * NW * 2 * KT * 4 * 64 <= 160 * 1024, "fk_product_kernel exceeds the gfx950 LDS");
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, j = lane & 15, g = lane >> 4;
  const int c = blockIdx.y, i0 = blockIdx.x * 32;
  const int* mem = order + offs[c];
  const int cpm = (k + 15) / 16, chunks = (offs[c + 1] - offs[c]) * cpm, q = (chunks + NW - 1) / NW;
  const int lo = wave * q < chunks ? wave * q : chunks, hi = lo + q < chunks ? lo + q : chunks;
  const bool vec = (R & 3) == 0 && (k & 3) == 0;         // every lane's four columns start on a 32-byte boundary and end inside the member
  geom_d4 acc[2][KT];
#pragma unroll
  for (int tl = 0; tl < 2; ++tl)
#pragma unroll
    for (int n = 0; n < KT; ++n) acc[tl][n] = geom_d4{0.0, 0.0, 0.0, 0.0};
  FkOperands<KT> o0, o1;
  fk_load<KT>(o0, G, Z, mem, lo, hi, cpm, i0, j, g, R, k, r, vec);
  for (int ch = lo; ch < hi; ch += 2) {                  // (a chunk past hi loads zeros: its MFMAs add nothing)
    fk_load<KT>(o1, G, Z, mem, ch + 1, hi, cpm, i0, j, g, R, k, r, vec);
    fk_mma<KT>(acc, o0);
    fk_load<KT>(o0, G, Z, mem, ch + 2, hi, cpm, i0, j, g, R, k, r, vec);
    fk_mma<KT>(acc, o1);
  }
#pragma unroll
  for (int tl = 0; tl < 2; ++tl)
#pragma unroll
    for (int n = 0; n < KT; ++n)
#pragma unroll
      for (int x = 0; x < 4; ++x) red[wave][tl][n][x][lane] = acc[tl][n][x];
  __syncthreads();
  const long ld = (long)C * r;
  for (int e = t; e < 2 * KT * 4 * 64; e += NW * 64) {
    const int ln = e & 63, x = (e >> 6) & 3, n = (e >> 8) % KT, tl = (e >> 8) / KT;
    double v = red[0][tl][n][x][ln];
#pragma unroll
    for (int w = 1; w < NW; ++w) v += red[w][tl][n][x][ln];
    const int row = i0 + 16 * tl + (ln >> 4) + 4 * x, col = 16 * n + (ln & 15);
    if (row < R && col < r) S[(long)row * ld + (long)c * r + col] = v;
  }
}

// block i: a[i, c] = ||S[i-rows, c-block]||_F^2, a wave per cluster (lane-strided squares in element order, then the xor butterfly), and the member's
// wish: argmax_c a[i, c], the lowest c on a tie, if that exceeds its own cluster's by more than margin, else its own.  A degenerate member: NaN, -1
__global__ __launch_bounds__(256) void fk_affinity_kernel(const double* S, const int* labels, const int* flags, double* aff, int* want, int k, int r, int C,
                                                          double margin) {
  const int i = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long ld = (long)C * r;
  const bool bad = flags[i] != 0;
  for (int c = wave; c < C; c += 4) {
    double sq = 0.0;
    if (!bad)
      for (int e = lane; e < k * r; e += 64) {
        const double v = S[((long)i * k + e / r) * ld + (long)c * r + e % r];
        sq += v * v;
      }
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
    if (lane == 0) aff[(long)i * C + c] = bad ? nan64() : sq;
  }
  __syncthreads();                                      // (orders this workgroup's global stores for its own reads)
  if (t == 0) {
    int w = -1;
    if (!bad) {
      const int own = labels[i];
      int best = 0;
      double bv = aff[(long)i * C];
      for (int c = 1; c < C; ++c) { const double v = aff[(long)i * C + c]; if (v > bv) { bv = v; best = c; } }
      w = (best != own && bv > aff[(long)i * C + own] + margin) ? best : own;
    }
    want[i] = w;
  }
}

// one workgroup: J = sum_i (r - a[i, label_i]) (thread-strided partial sums, block_sum: a function of B only); with apply, the keep rule -- a
// cluster none of whose members wants to stay keeps the one of largest affinity to it, the lowest index on a tie -- the new labels, the counts and the
// clusters whose member set changed
__global__ __launch_bounds__(256) void fk_move_kernel(const double* aff, int* want, int* labels, const int* order, const int* offs, int* changed, FkHead* head,
                                                      int B, int C, int r, int apply) {
  __shared__ double red[4];
  const int t = threadIdx.x;
  double part = 0.0;
  for (int i = t; i < B; i += 256) { const int c = labels[i]; if (c >= 0) part += (double)r - aff[(long)i * C + c]; }
  const double J = block_sum<256>(part, red);
  double kept = 0.0, moved = 0.0;
  for (int c = t; c < C; c += 256) changed[c] = 0;
  if (apply) {
    for (int c = t; c < C; c += 256) {
      const int lo = offs[c], hi = offs[c + 1];
      int stay = 0, best = -1;
      double bv = 0.0;
      for (int e = lo; e < hi; ++e) {
        const int i = order[e];
        if (want[i] == c) stay += 1;
        const double v = aff[(long)i * C + c];
        if (best < 0 || v > bv) { bv = v; best = i; }
      }
      if (stay == 0 && best >= 0) { want[best] = c; kept += 1.0; }
    }
  }
  __syncthreads();
  if (apply) {
    for (int i = t; i < B; i += 256) {
      const int o = labels[i], w = want[i];
      if (o >= 0 && w != o) { changed[o] = 1; changed[w] = 1; labels[i] = w; moved += 1.0; }      // (a benign race: every writer stores 1)
    }
  }
  const double nk = block_sum<256>(kept, red), nm = block_sum<256>(moved, red);
  if (t == 0) { head->J = J; head->kept = (int)nk; head->moved = (int)nm; }
}

// ------------------------------------------------------------------------------------------------------------ finish: coefficients on the given rows
// block i: Out[member i's rows][col0 + a] = (Z blockdiag(W))_i, sum_{x >= b} Z[i k + x][a] W_i[x][b]: the coefficients of its centre's rows on the
// rows of X as given.  one: Out is [R][C r] and col0 = label r; otherwise Out is [C][R][r], cluster by cluster.  Out is zero elsewhere (cleared before)
__global__ __launch_bounds__(256) void fk_coef_kernel(const double* Z, const double* W, const int* labels, double* Out, int k, int r, int C, long R, int one) {
  const int i = blockIdx.x, c = labels[i];
  if (c < 0) return;
  const double* Wi = W + (long)i * k * k;
  const double* Zi = Z + (long)i * k * r;
  for (int e = threadIdx.x; e < k * r; e += 256) {
    const int b = e / r, a = e % r;
    double s = 0.0;
    for (int x = b; x < k; ++x) s += Zi[x * r + a] * Wi[x * k + b];
    if (one) Out[((long)i * k + b) * ((long)C * r) + (long)c * r + a] = s;
    else Out[(long)c * R * r + ((long)i * k + b) * r + a] = s;
  }
}

// ------------------------------------------------------------------------------------------------------------ host side
size_t flag_kmeans_scratch_bytes(long B, int k, long N, long C, int r) {
  FkLayout l;
  return fk_layout(B, k, N, C, r, l) ? l.total : 0;
}

size_t flag_kmeans_host_bytes(long B, int k, long N, long C, int r) {
  FkLayout l;
  return fk_layout(B, k, N, C, r, l) ? l.host_bytes : 0;
}

const double* flag_kmeans_affinity(long B, int k, long N, long C, int r, const void* scratch) {
  FkLayout l;
  return fk_layout(B, k, N, C, r, l) ? (const double*)((const char*)scratch + l.aff) : nullptr;
}

int launch_flag_kmeans_init(const float* X, long B, int k, long N, long C, int r, const int32_t* seeds, int n_seeds, void* scratch, size_t scratch_bytes,
                            hipStream_t st) {
  FkLayout l;
  if (fk_check("dpb_flag_kmeans_init", B, k, N, C, r, scratch, scratch_bytes, l) != 0) return -1;
  if (n_seeds != 1 && n_seeds != C) { set_error("dpb_flag_kmeans_init: n_seeds=%d must be 1 (farthest-first from seeds[0]) or C=%ld", n_seeds, C); return -1; }
  for (int a = 0; a < n_seeds; ++a) {
    if (seeds[a] < 0 || seeds[a] >= B) { set_error("dpb_flag_kmeans_init: seeds[%d]=%d outside [0,%ld)", a, seeds[a], B); return -1; }
    for (int b = 0; b < a; ++b)
      if (seeds[b] == seeds[a]) { set_error("dpb_flag_kmeans_init: seeds[%d] = seeds[%d] = %d: the seeds must be distinct", b, a, seeds[a]); return -1; }
  }
  const FkPtrs p = fk_ptrs(scratch, l);
  if (launch_whitened_gram(X, B, k, N, p.G, p.W, p.flags, st) != 0) return -1;
  DPB_CHECK(hipMemsetAsync(p.seeds, 0, (size_t)C * sizeof(int), st));
  DPB_CHECK(hipMemcpyAsync(p.seeds, seeds, (size_t)n_seeds * sizeof(int), hipMemcpyHostToDevice, st));
  DPB_CHECK(hipStreamSynchronize(st));                   // (the host list may go out of scope; the one synchronisation of the run's set-up)
  const dim3 gb((unsigned)B), one(1), t256(256);
  for (int t = 0; t < (int)C; ++t) {
    DPB_LAUNCH(fk_seed_dist_kernel, gb, t256, 0, st, p.G, p.flags, p.seeds, t, p.dmin, p.labels, (long)(B * k), k);
    if (n_seeds == 1 && t + 1 < C) DPB_LAUNCH(fk_seed_pick_kernel, one, t256, 0, st, p.dmin, p.seeds, t, (int)B);
  }
  DPB_LAUNCH(fk_lists_kernel, one, t256, 0, st, p.labels, p.flags, p.sizes, p.offs, p.order, p.changed, p.head, (int)B, (int)C, 1);
  DPB_CHECK(hipGetLastError());
  return 0;
}

int launch_flag_kmeans_gather(long B, int k, long N, long C, int r, int c, int n_c, double* Gc, void* scratch, size_t scratch_bytes, hipStream_t st) {
  FkLayout l;
  if (fk_check("dpb_flag_kmeans_gather", B, k, N, C, r, scratch, scratch_bytes, l) != 0) return -1;
  if (c < 0 || c >= C || n_c < 1 || n_c > B) { set_error("dpb_flag_kmeans_gather: c=%d outside [0,%ld) or n_c=%d outside [1,B]", c, C, n_c); return -1; }
  if ((uintptr_t)Gc % 32) { set_error("dpb_flag_kmeans_gather: Gc must be 32-byte aligned"); return -1; }
  const FkPtrs p = fk_ptrs(scratch, l);
  DPB_LAUNCH(fk_gather_kernel, dim3((unsigned)n_c, (unsigned)n_c), dim3(256), 0, st, p.G, p.order, p.offs, c, n_c, Gc, (long)(B * k), k);
  DPB_CHECK(hipGetLastError());
  return 0;
}

int launch_flag_kmeans_set_centre(long B, int k, long N, long C, int r, int c, int n_c, const double* Ct, void* scratch, size_t scratch_bytes, hipStream_t st) {
  FkLayout l;
  if (fk_check("dpb_flag_kmeans_set_centre", B, k, N, C, r, scratch, scratch_bytes, l) != 0) return -1;
  if (c < 0 || c >= C || n_c < 1 || n_c > B) { set_error("dpb_flag_kmeans_set_centre: c=%d outside [0,%ld) or n_c=%d outside [1,B]", c, C, n_c); return -1; }
  const FkPtrs p = fk_ptrs(scratch, l);
  DPB_LAUNCH(fk_scatter_kernel, dim3((unsigned)n_c), dim3(256), 0, st, Ct, p.order, p.offs, c, n_c, p.Z, k, r);
  DPB_CHECK(hipGetLastError());
  return 0;
}

int launch_flag_kmeans_assign(long B, int k, long N, long C, int r, int apply, void* scratch, size_t scratch_bytes, hipStream_t st) {
  FkLayout l;
  if (fk_check("dpb_flag_kmeans_assign", B, k, N, C, r, scratch, scratch_bytes, l) != 0) return -1;
  const FkPtrs p = fk_ptrs(scratch, l);
  const int R = (int)(B * k);
  const dim3 grid((R + 31) / 32, (unsigned)C), gb((unsigned)B), one(1), t256(256);
  DPB_BY_TILES(r, DPB_LAUNCH((fk_product_kernel<KT, 8>), grid, dim3(512), 0, st, p.G, p.Z, p.S, p.order, p.offs, R, k, r, (int)C));
  DPB_LAUNCH(fk_affinity_kernel, gb, t256, 0, st, p.S, p.labels, p.flags, p.aff, p.want, k, r, (int)C, 1e-12 * r);
  DPB_LAUNCH(fk_move_kernel, one, t256, 0, st, p.aff, p.want, p.labels, p.order, p.offs, p.changed, p.head, (int)B, (int)C, r, apply ? 1 : 0);
  if (apply) DPB_LAUNCH(fk_lists_kernel, one, t256, 0, st, p.labels, p.flags, p.sizes, p.offs, p.order, p.changed, p.head, (int)B, (int)C, 0);
  DPB_CHECK(hipGetLastError());
  return 0;
}

int launch_flag_kmeans_finish(const float* X, long B, int k, long N, long C, int r, float* Y, void* scratch, size_t scratch_bytes, hipStream_t st) {
  FkLayout l;
  if (fk_check("dpb_flag_kmeans_finish", B, k, N, C, r, scratch, scratch_bytes, l) != 0) return -1;
  const FkPtrs p = fk_ptrs(scratch, l);
  const int R = (int)(B * k);
  const int one = C * r <= 64 ? 1 : 0;
  DPB_CHECK(hipMemsetAsync(p.S, 0, (size_t)R * C * r * sizeof(double), st));      // (S is free after the last assignment: the zero-padded coefficients take it)
  DPB_LAUNCH(fk_coef_kernel, dim3((unsigned)B), dim3(256), 0, st, p.Z, p.W, p.labels, p.S, k, r, (int)C, (long)R, one);
  if (one) {
    if (launch_coef_stream(X, p.S, Y, R, (int)(C * r), N, st) != 0) return -1;
  } else {
    for (long c = 0; c < C; ++c)
      if (launch_coef_stream(X, p.S + c * R * r, Y + c * r * N, R, r, N, st) != 0) return -1;
  }
  DPB_CHECK(hipGetLastError());
  return 0;
}

}  // namespace dpb
