// Parallel transport of principal directions between local tangent spaces (run_edit_parallel_transport, src/modules/edit.py:782-948): the source's
// h-space direction u_src[pc] is expressed in the target's h-space basis and carried to x-space through the target's own (u, vT) pairing,
//   c[d][p][q] = <uhat_dst[d][q], uhat_src[pc_p]>,     w[d][p][:] = sum_q c[d][p][q] vhat_dst[d][q][:],     vk = w / ||w||_2,
// with uhat / vhat the rows scaled to unit length.  fp32 in / fp32 out; D targets per call, k <= 128 rows per basis, N_x up to 196 608 and beyond.
//
// Nothing of size N is normalised or copied.  The overlaps u_dst u_src^T come from the exact fp64 cross-Gram of angles.hip, the row sums of squares from
// a fixed-order fp64 reduction (rowsumsq_kernel), c is formed in fp64 (coef_kernel) and handed to the streaming kernel already divided by the vT row
// norm and rounded ONCE to fp32.  stream_kernel reads vT_dst[d] once from memory (a workgroup's 1024-column chunk is re-read from L2 for every further tile
// of eight directions), accumulates in fp32 with one v_fma_f32 per term in the order q = 0 .. k-1, writes w into vk and the fp64 sum of squares of what it
// wrote per (d, p, chunk); norm_kernel adds the chunks in chunk order and scale_kernel brings vk to unit length in place.
// Reproducibility: no atomics; every sum is one fixed chain whose shape depends on k, N_h and N_x only, never on D, P, the position of a target in the
// stack or the alignment of the pointers (the 16-byte and the 4-byte load paths give every thread the same elements in the same order).
#include "kernels.h"
#include "geom.h"

namespace dpb {

constexpr int TR_NT = 256;                 // threads per workgroup
constexpr int TR_CHUNK = TR_NT * 4;        // columns of N_x per workgroup of the streaming kernel: four per thread
constexpr int TR_PT = 8;                   // directions per register tile of the streaming kernel (8 x 4 fp32 accumulators per thread)
constexpr int TR_MAX_TARGETS = 65535;      // a grid axis

struct TransportPcs { unsigned char pc[ORTH_MAX_RANK]; };      // the host's list travels as a kernel argument (entries < k <= 128)

// ss[r] = sum_n X[r][n]^2 in fp64, one workgroup per row.  Thread t adds the elements of its groups of four (group g = t, t + 256, ...) in index order
// into ONE accumulator; the 256 accumulators meet in block_sum: a chain that depends on N only.
__global__ __launch_bounds__(TR_NT) void rowsumsq_kernel(const float* X, long N, double* ss, int vec) {
  __shared__ double red[TR_NT / 64];
  const float* row = X + (long)blockIdx.x * N;
  double acc = 0.0;
  for (long n = (long)threadIdx.x * 4; n < N; n += TR_CHUNK) {
    const float4 v = load4(row, n, N, vec);
    acc += (double)v.x * (double)v.x;
    acc += (double)v.y * (double)v.y;
    acc += (double)v.z * (double)v.z;
    acc += (double)v.w * (double)v.w;
  }
  const double s = block_sum<TR_NT>(acc, red);
  if (threadIdx.x == 0) ss[blockIdx.x] = s;
}

// One thread per (d, p): c[q] = G[d][q][pc] / (||u_dst[d][q]|| ||u_src[pc]||) in fp64, q in order.  Writes coef and coef_norm (fp32) and the streaming
// kernel's coefficients a[d][p][q] = c[q] / ||vT_dst[d][q]||.  The degenerate rule: a zero / non-finite source row pc, a zero / non-finite row of the
// target's u or vT, or c == 0 exactly make coef, coef_norm and a (hence vk) of this (d, p) NaN.
__global__ __launch_bounds__(TR_NT) void coef_kernel(const double* G, const double* ss_src, const double* ss_u, const double* ss_v, TransportPcs pcs,
                                                     int D, int P, int k, float* coef, float* coef_norm, float* a) {
  const long e = (long)blockIdx.x * TR_NT + threadIdx.x;
  if (e >= (long)D * P) return;
  const long d = e / P;
  const int p = (int)(e % P), pc = pcs.pc[p];
  const double s0 = ss_src[pc];
  bool bad = !(s0 > 0.0) || !(s0 < 1.7e308);
  for (int q = 0; q < k; ++q) {
    const double su = ss_u[d * k + q], sv = ss_v[d * k + q];
    if (!(su > 0.0) || !(su < 1.7e308) || !(sv > 0.0) || !(sv < 1.7e308)) bad = true;
  }
  const double r0 = 1.0 / sqrt(s0);
  double nn = 0.0;
  if (!bad)
    for (int q = 0; q < k; ++q) {
      const double c = G[(d * k + q) * k + pc] / sqrt(ss_u[d * k + q]) * r0;
      nn += c * c;
    }
  if (!(nn > 0.0) || !(nn < 1.7e308)) bad = true;                     // c == 0 exactly (or a non-finite overlap)
  const float nanf_ = __uint_as_float(0x7fc00000u);
  float* co = coef + e * k;
  float* ao = a + e * k;
  for (int q = 0; q < k; ++q) {
    if (bad) { co[q] = nanf_; ao[q] = nanf_; continue; }
    const double c = G[(d * k + q) * k + pc] / sqrt(ss_u[d * k + q]) * r0;
    co[q] = (float)c;
    ao[q] = (float)(c / sqrt(ss_v[d * k + q]));
  }
  coef_norm[e] = bad ? nanf_ : (float)sqrt(nn);
}

// grid (chunks of N_x, D).  w[d][p][n] = sum_q a[d][p][q] vT[d][q][n]: thread t owns columns chunk * 1024 + 4t .. + 3, for TR_PT directions at a time;
// the tile's coefficients sit in LDS as [q][TR_PT] (two broadcast 16-byte reads per q).  part[d][p][chunk] = the fp64 sum of squares of the w written.
__global__ __launch_bounds__(TR_NT) void stream_kernel(const float* vT, const float* a, float* w, double* part, int P, int k, long N, long chunks, int vec) {
  __shared__ __attribute__((aligned(16))) float cs[ORTH_MAX_RANK * TR_PT];
  __shared__ double red[TR_NT / 64];
  const long d = blockIdx.y, chunk = blockIdx.x;
  const float* V = vT + d * k * N;
  const long n = chunk * TR_CHUNK + (long)threadIdx.x * 4;
  for (int p0 = 0; p0 < P; p0 += TR_PT) {
    __syncthreads();                                                 // the previous tile's reads of cs are over
    for (int e = threadIdx.x; e < k * TR_PT; e += TR_NT) {
      const int q = e / TR_PT, j = e % TR_PT;
      cs[e] = p0 + j < P ? a[(d * P + p0 + j) * k + q] : 0.f;
    }
    __syncthreads();
    float4 acc[TR_PT];
#pragma unroll
    for (int j = 0; j < TR_PT; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int q = 0; q < k; ++q) {
      const float4 v = load4(V + (long)q * N, n, N, vec);
      const float4 c0 = *reinterpret_cast<const float4*>(&cs[q * TR_PT]);
      const float4 c1 = *reinterpret_cast<const float4*>(&cs[q * TR_PT + 4]);
      const float c[TR_PT] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
#pragma unroll
      for (int j = 0; j < TR_PT; ++j) {
        acc[j].x = __builtin_fmaf(c[j], v.x, acc[j].x);
        acc[j].y = __builtin_fmaf(c[j], v.y, acc[j].y);
        acc[j].z = __builtin_fmaf(c[j], v.z, acc[j].z);
        acc[j].w = __builtin_fmaf(c[j], v.w, acc[j].w);
      }
    }
#pragma unroll
    for (int j = 0; j < TR_PT; ++j) {
      if (p0 + j >= P) break;                                        // uniform
      float* o = w + (d * P + p0 + j) * N;
      double s = 0.0;                                                // columns past N hold zeros: they add nothing and are not stored
      s += (double)acc[j].x * (double)acc[j].x;
      s += (double)acc[j].y * (double)acc[j].y;
      s += (double)acc[j].z * (double)acc[j].z;
      s += (double)acc[j].w * (double)acc[j].w;
      store4(o, n, N, vec, acc[j]);
      s = block_sum<TR_NT>(s, red);
      if (threadIdx.x == 0) part[(d * P + p0 + j) * chunks + chunk] = s;
    }
  }
}

// one thread per (d, p): ||w||^2 = the chunks' partial sums in chunk order; scale = 1 / ||w|| (inf for w = 0: vk becomes NaN; NaN stays NaN)
__global__ __launch_bounds__(TR_NT) void norm_kernel(const double* part, long rows, long chunks, float* scale) {
  const long e = (long)blockIdx.x * TR_NT + threadIdx.x;
  if (e >= rows) return;
  double s = 0.0;
  for (long c = 0; c < chunks; ++c) s += part[e * chunks + c];
  scale[e] = (float)(1.0 / sqrt(s));
}

// grid (chunks of N_x, D * P): vk <- vk * scale, in place
__global__ __launch_bounds__(TR_NT) void scale_kernel(float* w, const float* scale, long N, int vec) {
  const long r = blockIdx.y;
  const float s = scale[r];
  float* o = w + r * N;
  const long n = (long)blockIdx.x * TR_CHUNK + (long)threadIdx.x * 4;
  if (n >= N) return;
  if (vec) {
    float4 v = *reinterpret_cast<float4*>(o + n);
    v.x *= s; v.y *= s; v.z *= s; v.w *= s;
    *reinterpret_cast<float4*>(o + n) = v;
  } else {
    for (int i = 0; i < 4 && n + i < N; ++i) o[n + i] *= s;
  }
}

// ------------------------------------------------------------------------------------------------------------ host side
namespace {
struct TransportLayout { size_t g = 0, ss_src = 0, ss_u = 0, ss_v = 0, a = 0, part = 0, scale = 0, total = 0; long chunks = 0; };
bool transport_layout(long D, int P, int k, long Nh, long Nx, TransportLayout& l) {
  if (D < 1 || D > TR_MAX_TARGETS || k < 1 || k > ORTH_MAX_RANK || P < 1 || P > k || Nh < 1 || Nx < 1) return false;
  ScratchCarver s;
  l.chunks = (Nx + TR_CHUNK - 1) / TR_CHUNK;
  l.g = s.take((size_t)D * k * k * sizeof(double));
  l.ss_src = s.take((size_t)k * sizeof(double));
  l.ss_u = s.take((size_t)D * k * sizeof(double));
  l.ss_v = s.take((size_t)D * k * sizeof(double));
  l.a = s.take((size_t)D * P * k * sizeof(float));
  l.part = s.take((size_t)D * P * (size_t)l.chunks * sizeof(double));
  l.scale = s.take((size_t)D * P * sizeof(float));
  l.total = s.off;
  return true;
}
}  // namespace

size_t transport_scratch_bytes(long D, int P, int k, long Nh, long Nx) {
  TransportLayout l;
  return transport_layout(D, P, k, Nh, Nx, l) ? l.total : 0;
}

int launch_rowsumsq(const float* X, long rows, long N, double* ss, hipStream_t st) {
  if (rows < 1 || rows > 0x7fffffffL || N < 1) { set_error("dpb_row_sumsq: rows=%ld outside [1,2^31) or N=%ld < 1", rows, N); return -1; }
  const int vec = (N % 4 == 0 && (uintptr_t)X % 16 == 0) ? 1 : 0;
  DPB_LAUNCH(rowsumsq_kernel, dim3((unsigned)rows), dim3(TR_NT), 0, st, X, N, ss, vec);
  DPB_CHECK(hipGetLastError());
  return 0;
}

int launch_transport_directions(const float* u_src, const float* u_dst, const float* vT_dst, const int32_t* pcs, int P, long D, int k, long Nh, long Nx,
                                float* vk, float* coef, float* coef_norm, void* scratch, size_t scratch_bytes, hipStream_t st) {
  TransportLayout l;
  if (!transport_layout(D, P, k, Nh, Nx, l)) {
    set_error("dpb_transport_directions: D=%ld outside [1,%d], k=%d outside [1,%d], P=%d outside [1,k], or N_h=%ld, N_x=%ld < 1", D, TR_MAX_TARGETS, k,
              ORTH_MAX_RANK, P, Nh, Nx);
    return -1;
  }
  TransportPcs pc;
  for (int p = 0; p < P; ++p) {
    if (pcs[p] < 0 || pcs[p] >= k) { set_error("dpb_transport_directions: pcs[%d]=%d outside [0,%d)", p, (int)pcs[p], k); return -1; }
    pc.pc[p] = (unsigned char)pcs[p];
  }
  if (check_scratch("dpb_transport_directions", scratch, scratch_bytes, l.total, "dpb_transport_scratch_bytes(%ld, %d, %d, %ld, %ld)", D, P, k, Nh, Nx) != 0)
    return -1;
  char* base = (char*)scratch;
  double* G = (double*)(base + l.g);
  double* ss_src = (double*)(base + l.ss_src);
  double* ss_u = (double*)(base + l.ss_u);
  double* ss_v = (double*)(base + l.ss_v);
  float* a = (float*)(base + l.a);
  double* part = (double*)(base + l.part);
  float* scale = (float*)(base + l.scale);
  // h-space side: G[d][q][j] = <u_dst[d][q], u_src[j]>, an entry does not depend on the rows around it (dpb_cross_gram); as many targets per launch as
  // its row limit takes
  const long per = (long)(65535L * 64 / k);
  for (long d0 = 0; d0 < D; d0 += per) {
    const long nd = D - d0 < per ? D - d0 : per;
    if (launch_cross_gram(u_dst + d0 * k * Nh, u_src, G + d0 * k * k, (int)(nd * k), k, Nh, st) != 0) return -1;
  }
  const int vh = (Nh % 4 == 0 && (uintptr_t)u_src % 16 == 0) ? 1 : 0, vhd = (Nh % 4 == 0 && (uintptr_t)u_dst % 16 == 0) ? 1 : 0;
  const int vx = (Nx % 4 == 0 && (uintptr_t)vT_dst % 16 == 0 && (uintptr_t)vk % 16 == 0) ? 1 : 0;
  DPB_LAUNCH(rowsumsq_kernel, dim3(k), dim3(TR_NT), 0, st, u_src, Nh, ss_src, vh);
  DPB_LAUNCH(rowsumsq_kernel, dim3((unsigned)(D * k)), dim3(TR_NT), 0, st, u_dst, Nh, ss_u, vhd);
  DPB_LAUNCH(rowsumsq_kernel, dim3((unsigned)(D * k)), dim3(TR_NT), 0, st, vT_dst, Nx, ss_v, vx);
  const long rows = D * P;
  const unsigned rb = (unsigned)((rows + TR_NT - 1) / TR_NT);
  DPB_LAUNCH(coef_kernel, dim3(rb), dim3(TR_NT), 0, st, G, ss_src, ss_u, ss_v, pc, (int)D, P, k, coef, coef_norm, a);
  DPB_LAUNCH(stream_kernel, dim3((unsigned)l.chunks, (unsigned)D), dim3(TR_NT), 0, st, vT_dst, a, vk, part, P, k, Nx, l.chunks, vx);
  DPB_LAUNCH(norm_kernel, dim3(rb), dim3(TR_NT), 0, st, part, rows, l.chunks, scale);
  // (grid.y <= 65535: the rows go through in slabs)
  for (long r0 = 0; r0 < rows; r0 += 65535) {
    const long nr = rows - r0 < 65535 ? rows - r0 : 65535;
    DPB_LAUNCH(scale_kernel, dim3((unsigned)l.chunks, (unsigned)nr), dim3(TR_NT), 0, st, vk + r0 * Nx, scale + r0, Nx, vx);
  }
  DPB_CHECK(hipGetLastError());
  return 0;
}

}  // namespace dpb
