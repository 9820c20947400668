// The h-space guidance edit (Kwon et al., "Diffusion models already have a semantic latent space": Asyrp; the reference's edit_ht == 'h_space_guidance',
// src/modules/edit.py:1232-1245, :1500-1513, whose h_space_guidance method it never defines): at every DDIM step of the guided interval the net runs
// twice, plain (e) and with the tap shifted by sigma c (e_s), and the two halves of the DDIM update take their own mix of the two,
//   d = e_s - e,  eP = e + gP d,  eD = e + gD d,  P = (x - eP sqrt(1-a)) / sqrt(a),  x' = sqrt(a') P + sqrt(1-a') eD        (eta = 0)
// (gP, gD) = (1, 0): Asyrp's asymmetric process; (1, 1): the plain DDIM step of the shifted net.  The U-Net passes are the engine's; this file holds
//   the asymmetric DDIM step   (x, e, e_s) -> x', optionally P, and per row (sum d^2, flag) in fp64;
//   the grouped tap shift      P(tap)[g xb + b] = P(tap)[b] + scale[g xb + b] u[dir[g xb + b]], the seam of dpb_forward_shift_groups.
// The step is fp32 in the operation order of ddim_kernel (elementwise.hip): d, eP and eD are formed first with one rounding each, so a row with d == 0
// or gP == gD == 0 is dpb_ddim_step on (x, e) bit for bit.  The sum of d^2 follows chain.hip: thread t of a workgroup adds the elements of its groups of
// four in index order in fp64, the 256 accumulators meet in block_sum, and a row's slices of HG_SLICE elements are added in slice order; no atomics, so a
// row's results are a function of the row and N only -- not of n, of the row's position in the stack or of the alignment of its pointers.
#include "kernels.h"
#include "geom.h"

namespace dpb {

namespace {

constexpr int HG_NT = 256;                  // threads per workgroup
constexpr int HG_GROUPS = 4;                // groups of four elements per thread and slice
constexpr int HG_SLICE = HG_NT * 4 * HG_GROUPS;   // elements of a row per workgroup: 4096
constexpr long HG_MAX_ROWS = 32768;         // rows per launch (gridDim.y)
constexpr int HGS_TP = 32, HGS_TC = 64;     // the tile of the tap shift: pixels x channels, as shift_tap_kernel

__device__ inline bool hg_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// elements j .. j+3 of a row of length N (j % 4 == 0, j < N), zeros past its end; al: the row pointer is 16-byte aligned
__device__ inline float4 hg_load4(const float* row, long j, long N, bool al) {
  if (al && j + 3 < N) return *reinterpret_cast<const float4*>(row + j);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  v.x = row[j];
  if (j + 1 < N) v.y = row[j + 1];
  if (j + 2 < N) v.z = row[j + 2];
  if (j + 3 < N) v.w = row[j + 3];
  return v;
}

__device__ inline void hg_store4(float* row, long j, long N, bool al, float4 v) {
  if (al && j + 3 < N) { *reinterpret_cast<float4*>(row + j) = v; return; }
  row[j] = v.x;
  if (j + 1 < N) row[j + 1] = v.y;
  if (j + 2 < N) row[j + 2] = v.z;
  if (j + 3 < N) row[j + 3] = v.w;
}

__device__ inline bool hg_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }   // false for NaN and +-inf

// part[b][slice] = (sum d^2 of the slice in fp64, number of non-finite elements of x, e and e_s in it)
__global__ __launch_bounds__(HG_NT) void hguide_partial_kernel(const float* x, const float* e, const float* es, long N, double* part) {
  __shared__ double red[HG_NT / 64];
  const int b = blockIdx.y, t = threadIdx.x;
  const long nsl = gridDim.x, off = (long)b * N;
  const bool alx = hg_aligned16(x + off), ale = hg_aligned16(e + off), als = hg_aligned16(es + off);
  double s2 = 0.0, bad = 0.0;
#pragma unroll
  for (int i = 0; i < HG_GROUPS; ++i) {
    const long j = (long)blockIdx.x * HG_SLICE + ((long)i * HG_NT + t) * 4;
    if (j < N) {
      const float4 xv = hg_load4(x + off, j, N, alx), ev = hg_load4(e + off, j, N, ale), sv = hg_load4(es + off, j, N, als);
      const float xi[4] = {xv.x, xv.y, xv.z, xv.w}, ei[4] = {ev.x, ev.y, ev.z, ev.w}, si[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double d = (double)(si[c] - ei[c]);          // the fp32 difference the step uses, widened
        s2 += d * d;
        if (!hg_finite(xi[c]) || !hg_finite(ei[c]) || !hg_finite(si[c])) bad += 1.0;
      }
    }
  }
  s2 = block_sum<HG_NT>(s2, red);
  bad = block_sum<HG_NT>(bad, red);
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
__global__ __launch_bounds__(HG_NT) void hguide_apply_kernel(const float* x, const float* e, const float* es, float* out, float* x0, long N, HgCoef k,
                                                             const double* part, double* stats) {
  __shared__ double row_s[2];
  const int b = blockIdx.y, t = threadIdx.x;
  const long nsl = gridDim.x, off = (long)b * N;
  if (t == 0) {
    double s2 = 0.0, bad = 0.0;
    for (long s = 0; s < nsl; ++s) {                       // slices in index order, the same chain in every workgroup of the row
      s2 += part[((long)b * nsl + s) * 2];
      bad += part[((long)b * nsl + s) * 2 + 1];
    }
    row_s[0] = s2; row_s[1] = bad;
  }
  __syncthreads();
  const bool bad = row_s[1] != 0.0;
  const float nanf_ = __builtin_nanf("");
  const bool alx = hg_aligned16(x + off), ale = hg_aligned16(e + off), als = hg_aligned16(es + off), alo = hg_aligned16(out + off),
             alp = x0 && hg_aligned16(x0 + off);
#pragma unroll
  for (int i = 0; i < HG_GROUPS; ++i) {
    const long j = (long)blockIdx.x * HG_SLICE + ((long)i * HG_NT + t) * 4;
    if (j >= N) continue;
    const float4 xv = hg_load4(x + off, j, N, alx), ev = hg_load4(e + off, j, N, ale), sv = hg_load4(es + off, j, N, als);
    const float xi[4] = {xv.x, xv.y, xv.z, xv.w}, ei[4] = {ev.x, ev.y, ev.z, ev.w}, si[4] = {sv.x, sv.y, sv.z, sv.w};
    float po[4], oo[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      hg_elem(xi[c], ei[c], si[c], k, po[c], oo[c]);
      if (bad) { po[c] = nanf_; oo[c] = nanf_; }
    }
    hg_store4(out + off, j, N, alo, make_float4(oo[0], oo[1], oo[2], oo[3]));
    if (x0) hg_store4(x0 + off, j, N, alp, make_float4(po[0], po[1], po[2], po[3]));
  }
  if (t == 0 && blockIdx.x == 0) { stats[(long)b * 2] = row_s[0]; stats[(long)b * 2 + 1] = bad ? 1.0 : 0.0; }
}

// The seam of dpb_forward_shift_groups: h holds the xb samples the prefix computed (rows 0 .. xb-1 of [groups xb][HW][C]); row g xb + b becomes
// h[b] + scale u[dir] for every group g.  As shift_tap_kernel, one block owns a tile of 32 pixels x 64 channels for ALL rows: sample b's tile is read
// into registers before any of its copies is written, and no other row is a source, so the in-place write of group 0 has no hazard.  rows: the
// (dir, scale) of samples b0 .. b0 + nb - 1, entry g nb + r for group g; a group-0 row with dir < 0 is its own source and is left alone.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void shift_tap_groups_kernel(T* h, const float* u, ShiftRows rows, int b0, int nb, int xb, int groups, int C, int Cv,
                                                               long HW) {
  constexpr int CPP = HGS_TC / VEC;                    // accesses per pixel of the tile
  constexpr int ITER = HGS_TP * CPP / 256;
  __shared__ float tile[HGS_TC][HGS_TP + 1];
  const long p0 = (long)blockIdx.x * HGS_TP;
  const int c0 = blockIdx.y * HGS_TC;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const long img = HW * (long)C;
  auto ld = [&](const T* p, float* o) {
    if constexpr (VEC == 1) o[0] = TT<T>::ld(p); else Vec<T>::load(p, o);
  };
  auto st = [&](T* p, const float* o) {
    if constexpr (VEC == 1) TT<T>::st(p, o[0]); else Vec<T>::store(p, o);
  };
  for (int r = 0; r < nb; ++r) {
    const int b = b0 + r;
    float src[ITER][VEC];
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
      const int q = it * 256 + threadIdx.x, pl = q / CPP, c = c0 + (q % CPP) * VEC;
#pragma unroll
      for (int el = 0; el < VEC; ++el) src[it][el] = 0.f;
      if (p0 + pl < HW && c < C) ld(h + (long)b * img + (p0 + pl) * C + c, src[it]);
    }
    for (int g = 0; g < groups; ++g) {
      const int dir = rows.dir[g * nb + r];
      const float sc = rows.scale[g * nb + r];
      if (dir < 0 && g == 0) continue;                     // unshifted row that is its own source: nothing to write (uniform over the block)
      if (dir >= 0) {
        __syncthreads();                                   // the tile of the row before has been read
        const float* ub = u + (long)dir * Cv * HW;
        for (int k = ty; k < HGS_TC; k += 8) {
          const int c = c0 + k;
          tile[k][tx] = (c < Cv && p0 + tx < HW) ? ub[(long)c * HW + p0 + tx] : 0.f;
        }
        __syncthreads();
      }
      T* hb = h + ((long)g * xb + b) * img;
#pragma unroll
      for (int it = 0; it < ITER; ++it) {
        const int q = it * 256 + threadIdx.x, pl = q / CPP, cl = (q % CPP) * VEC, c = c0 + cl;
        if (p0 + pl >= HW || c >= C) continue;
        float v[VEC];
#pragma unroll
        for (int el = 0; el < VEC; ++el) v[el] = src[it][el];
        if (dir >= 0) {
#pragma unroll
          for (int el = 0; el < VEC; ++el) v[el] += sc * tile[cl + el][pl];
        }
        st(hb + (p0 + pl) * C + c, v);
      }
    }
  }
}

template <typename T>
int shift_tap_groups_t(void* h, const float* u, const int* dir, const float* scale, int xb, int groups, int C, int Cv, long HW, hipStream_t st) {
  const dim3 grid((unsigned)((HW + HGS_TP - 1) / HGS_TP), (unsigned)((C + HGS_TC - 1) / HGS_TC));
  const int per = SHIFT_MAX_ROWS / groups;               // samples per launch: their rows of every group travel as kernel arguments
  for (int b0 = 0; b0 < xb; b0 += per) {
    ShiftRows rows;
    const int nb = std::min(per, xb - b0);
    for (int g = 0; g < groups; ++g)
      for (int r = 0; r < nb; ++r) { rows.dir[g * nb + r] = dir[g * xb + b0 + r]; rows.scale[g * nb + r] = scale[g * xb + b0 + r]; }
    if (C % TT<T>::CH == 0) DPB_LAUNCH((shift_tap_groups_kernel<T, TT<T>::CH>), grid, dim3(256), 0, st, (T*)h, u, rows, b0, nb, xb, groups, C, Cv, HW);
    else DPB_LAUNCH((shift_tap_groups_kernel<T, 1>), grid, dim3(256), 0, st, (T*)h, u, rows, b0, nb, xb, groups, C, Cv, HW);
    DPB_CHECK(hipGetLastError());
  }
  return 0;
}

}  // namespace

int launch_shift_tap_groups(int dtype, void* h, const float* u, const int* dir, const float* scale, int xb, int groups, int C, int Cv, long HW,
                            hipStream_t st) {
  if (xb < 1 || groups < 1 || C < 1 || Cv < 1 || Cv > C || HW < 1) { set_error("shift_tap_groups: empty or inconsistent problem"); return -1; }
  if (groups > SHIFT_MAX_ROWS) { set_error("shift_tap_groups: groups=%d above %d", groups, SHIFT_MAX_ROWS); return -1; }
  return DPB_DISPATCH_T(dtype, T, shift_tap_groups_t<T>(h, u, dir, scale, xb, groups, C, Cv, HW, st));
}

size_t ddim_step_asym_scratch_bytes(long n, long N) {
  if (n < 1 || N < 1) return 0;
  return (size_t)n * (size_t)((N + HG_SLICE - 1) / HG_SLICE) * 2 * sizeof(double);
}

int launch_ddim_step_asym(const float* x, const float* e, const float* es, float* out, float* x0, long n, long N, float a_t, float a_next, float gP,
                          float gD, double* stats, void* scratch, size_t scratch_bytes, hipStream_t st) {
  if (n < 1 || n > 0x7fffffffL) { set_error("ddim_step_asym: n=%ld rows outside [1, 2^31)", n); return -1; }
  if (N < 1) { set_error("ddim_step_asym: row length %ld < 1", N); return -1; }
  const long nsl = (N + HG_SLICE - 1) / HG_SLICE;
  if (nsl > 0x7fffffffL) { set_error("ddim_step_asym: row length %ld too large", N); return -1; }
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
    const dim3 grid((unsigned)nsl, (unsigned)rows), block(HG_NT);
    DPB_LAUNCH(hguide_partial_kernel, grid, block, 0, st, x + o, e + o, es + o, N, part + r0 * nsl * 2);
    DPB_LAUNCH(hguide_apply_kernel, grid, block, 0, st, x + o, e + o, es + o, out + o, x0 ? x0 + o : nullptr, N, k, (const double*)(part + r0 * nsl * 2),
               stats + r0 * 2);
  }
  DPB_CHECK(hipGetLastError());
  return 0;
}

}  // namespace dpb
