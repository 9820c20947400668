// noise.hip -- the perturbed batch of local PCA as one device step:  out[b][j] = x[j] + norm * g_b[j] / ||g_b||_2
// (reference: x + normalize_wrt_batch(torch.randn_like(x)), src/utils/utils.py:918-925, src/models/ddpm/diffusion.py:399-401).
//
// g_b is the caller's noise row, or generated here by Philox4x32-10 (Salmon et al., SC'11; the mapping to normals is written down in
// include/dpb.h next to dpb_perturb_unit): sample i's row is a function of (seed, i) only.  Two launches:
//   1. noise_sumsq_kernel  partial[b][s] = sum of g^2 over slice s (SLICE elements), fp64, one block per (slice, sample), a fixed order inside;
//   2. noise_apply_kernel  sums a sample's partials in slice order (every block the same way), regenerates g and writes out (and g itself
//                          when the caller asks for it) -- Philox is cheaper than a round trip through memory.
// The slice, the order inside it and the order of the slices are constants of the algorithm, not of the launch: the result for sample i is
// bitwise independent of B, `first` and the grid.  No atomics.  16-byte loads / stores when n % 4 == 0 and the pointers allow it, else
// element by element (the same arithmetic).  64-bit offsets throughout.
#include "common.h"
#include "kernels.h"

namespace dpb {

namespace {

constexpr int NOISE_THREADS = 256;
constexpr int NOISE_GROUPS = 4;                                  // groups of 4 elements per thread and slice
constexpr long NOISE_SLICE = 4L * NOISE_THREADS * NOISE_GROUPS;  // 4096 elements

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&o)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// u = ((w >> 9) + 0.5) * 2^-23: an odd multiple of 2^-24 below 1 -- 24 significant bits, exact in fp32, never 0, never 1
__device__ __forceinline__ float unit_open(uint32_t w) { return ((float)(w >> 9) + 0.5f) * 0x1p-23f; }

// the four normals of elements 4c .. 4c+3 of sample `idx`: Box-Muller on the word pairs (w0, w1) and (w2, w3)
__device__ __forceinline__ void normal4(uint64_t seed, uint64_t idx, uint64_t c, float (&g)[4]) {
  uint32_t w[4];
  philox4x32_10((uint32_t)idx, (uint32_t)(idx >> 32), (uint32_t)c, (uint32_t)(c >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), w);
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float r = sqrtf(-2.f * logf(unit_open(w[2 * p])));
    float sn, cs;
    sincospif(2.f * unit_open(w[2 * p + 1]), &sn, &cs);
    g[2 * p] = r * cs;
    g[2 * p + 1] = r * sn;
  }
}

// g of group c (elements 4c .. 4c+3; elements >= n read as 0) of sample b
template <bool VEC>
__device__ __forceinline__ void load_g(const float* noise, uint64_t seed, uint64_t idx, long row, long c, long n, float (&g)[4]) {
  if (noise) {
    if (VEC) {
      const float4 v = *(const float4*)(noise + row + 4 * c);
      g[0] = v.x; g[1] = v.y; g[2] = v.z; g[3] = v.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) g[i] = 4 * c + i < n ? noise[row + 4 * c + i] : 0.f;
    }
  } else {
    normal4(seed, idx, (uint64_t)c, g);
    if (!VEC) {
#pragma unroll
      for (int i = 0; i < 4; ++i) g[i] = 4 * c + i < n ? g[i] : 0.f;
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(NOISE_THREADS) void noise_sumsq_kernel(const float* noise, uint64_t seed, int64_t first, long n, double* partial) {
  __shared__ double red[NOISE_THREADS];
  const int b = blockIdx.y, t = threadIdx.x;
  const long nsl = gridDim.x, ng = (n + 3) / 4, row = (long)b * n;
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < NOISE_GROUPS; ++i) {
    const long c = (long)blockIdx.x * (NOISE_SLICE / 4) + (long)i * NOISE_THREADS + t;
    if (c < ng) {
      float g[4];
      load_g<VEC>(noise, seed, (uint64_t)(first + b), row, c, n, g);
      acc += (double)g[0] * g[0]; acc += (double)g[1] * g[1]; acc += (double)g[2] * g[2]; acc += (double)g[3] * g[3];
    }
  }
  red[t] = acc;
  __syncthreads();
  for (int s = NOISE_THREADS / 2; s > 0; s >>= 1) {          // fixed tree: the same pairs whatever the launch
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  if (t == 0) partial[(long)b * nsl + blockIdx.x] = red[0];
}

template <bool VEC>
__global__ __launch_bounds__(NOISE_THREADS) void noise_apply_kernel(const float* x, const float* noise, uint64_t seed, int64_t first, long n, float norm,
                                                                    const double* partial, float* out, float* noise_out) {
  __shared__ float scale_s;
  const int b = blockIdx.y, t = threadIdx.x;
  const long nsl = gridDim.x, ng = (n + 3) / 4, row = (long)b * n;
  if (t == 0) {
    double ss = 0.0;
    for (long s = 0; s < nsl; ++s) ss += partial[(long)b * nsl + s];      // slices in index order
    scale_s = (float)((double)norm / sqrt(ss));
  }
  __syncthreads();
  const float scale = scale_s;
#pragma unroll
  for (int i = 0; i < NOISE_GROUPS; ++i) {
    const long c = (long)blockIdx.x * (NOISE_SLICE / 4) + (long)i * NOISE_THREADS + t;
    if (c >= ng) continue;
    float g[4];
    load_g<VEC>(noise, seed, (uint64_t)(first + b), row, c, n, g);
    if (VEC) {
      const float4 xv = *(const float4*)(x + 4 * c);
      float4 o;
      o.x = __fmaf_rn(scale, g[0], xv.x); o.y = __fmaf_rn(scale, g[1], xv.y); o.z = __fmaf_rn(scale, g[2], xv.z); o.w = __fmaf_rn(scale, g[3], xv.w);
      *(float4*)(out + row + 4 * c) = o;
      if (noise_out) *(float4*)(noise_out + row + 4 * c) = make_float4(g[0], g[1], g[2], g[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long j = 4 * c + k;
        if (j < n) {
          out[row + j] = __fmaf_rn(scale, g[k], x[j]);
          if (noise_out) noise_out[row + j] = g[k];
        }
      }
    }
  }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

size_t perturb_scratch_bytes(int B, long n) {
  if (B < 1 || n < 1) return 0;
  return (size_t)B * (size_t)((n + NOISE_SLICE - 1) / NOISE_SLICE) * sizeof(double);
}

int launch_perturb_unit(const float* x, const float* noise, uint64_t seed, int64_t first, int B, long n, float norm, float* out, float* noise_out,
                        void* scratch, size_t scratch_bytes, hipStream_t st) {
  if (B < 1 || B > 65535) { set_error("perturb_unit: B=%d outside [1, 65535]", B); return -1; }
  if (n < 1) { set_error("perturb_unit: n=%ld < 1", n); return -1; }
  const long nsl = (n + NOISE_SLICE - 1) / NOISE_SLICE;
  if (nsl > 0x7fffffffL) { set_error("perturb_unit: n=%ld too large", n); return -1; }
  if (first < 0 || first > INT64_MAX - B) { set_error("perturb_unit: first=%lld invalid", (long long)first); return -1; }
  if (scratch_bytes < perturb_scratch_bytes(B, n)) {
    set_error("perturb_unit: scratch of %zu bytes, dpb_perturb_scratch_bytes(%d, %ld) = %zu", scratch_bytes, B, n, perturb_scratch_bytes(B, n));
    return -1;
  }
  if ((uintptr_t)scratch & 7) { set_error("perturb_unit: scratch must be 8-byte aligned"); return -1; }
  const bool vec = n % 4 == 0 && al16(x) && al16(out) && (!noise || al16(noise)) && (!noise_out || al16(noise_out));
  const dim3 grid((unsigned)nsl, (unsigned)B), block(NOISE_THREADS);
  double* partial = (double*)scratch;
  if (vec) {
    DPB_LAUNCH(noise_sumsq_kernel<true>, grid, block, 0, st, noise, seed, first, n, partial);
    DPB_LAUNCH(noise_apply_kernel<true>, grid, block, 0, st, x, noise, seed, first, n, norm, (const double*)partial, out, noise_out);
  } else {
    DPB_LAUNCH(noise_sumsq_kernel<false>, grid, block, 0, st, noise, seed, first, n, partial);
    DPB_LAUNCH(noise_apply_kernel<false>, grid, block, 0, st, x, noise, seed, first, n, norm, (const double*)partial, out, noise_out);
  }
  DPB_CHECK(hipGetLastError());
  return 0;
}

}  // namespace dpb
