// HBM-bound elementwise kernels: GEGLU (primal/tangent/adjoint), SiLU, accumulate, channel-window copies,
// NCHW<->NHWC boundary transposes, 2x2 pooling / nearest upsampling (each the other's adjoint), DDIM step.
// All use 16-byte chunks per lane and grid-stride loops.
#include "kernels.h"

namespace dpb {

static inline unsigned grid_for(long n) {
  long b = (n + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 16384 ? 16384 : b));
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void geglu_kernel(GegluArgs a, long nrows) {
  constexpr int CH = TT<T>::CH;
  const int fch = a.F / CH;
  const long total = nrows * fch;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long row = idx / fch;
    const int c = (int)(idx - row * fch) * CH;
    long prow = row;
    if (MODE != MODE_PRIMAL) {
      long j = row / a.rows_per_sample, l = row - j * a.rows_per_sample;
      prow = (j / a.kps) * a.rows_per_sample + l;
    }
    // column of a-unit c inside a [..][2F] row, and the distance to its gate: plain layout (a | g halves) or 64-blocks interleaved
    const int ca = a.il ? ((c >> 6) << 7) + (c & 63) : c, dg_ = a.il ? 64 : a.F;
    const T* hp = (const T*)a.h + prow * 2 * a.F;
    float av[CH], gv[CH], o[CH];
    Vec<T>::load(hp + ca, av);
    Vec<T>::load(hp + ca + dg_, gv);
    // The primal pass REPLACES (a, g) in h by the two factors every tangent / adjoint pass needs,
    //   G1 = gelu(g)  (in a's slot)   and   G2 = a * gelu'(g)  (in g's slot),
    // so that  dy = da*G1 + dg*G2  and  (ga, gg) = gy * (G1, G2)  cost two FMAs per element -- cheap enough to live in GEMM epilogues
    // (epilogue.h); h is read by nothing else after this kernel.
    if (MODE == MODE_PRIMAL) {
      float g1[CH], g2[CH];
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        const float er = erff(gv[e] * 0.70710678118654752f);
        g1[e] = 0.5f * gv[e] * (1.f + er);
        g2[e] = av[e] * (0.5f * (1.f + er) + gv[e] * 0.39894228040143268f * __expf(-0.5f * gv[e] * gv[e]));
        o[e] = av[e] * g1[e];
      }
      Vec<T>::store((T*)a.y + row * a.F + c, o);
      if (a.stash) {
        T* hw = (T*)a.h + prow * 2 * a.F;
        Vec<T>::store(hw + ca, g1);
        Vec<T>::store(hw + ca + dg_, g2);
      }
    } else if (MODE == MODE_TANGENT) {
      const T* dp = (const T*)a.d + row * 2 * a.F;
      float da[CH], dg[CH];
      Vec<T>::load(dp + ca, da);
      Vec<T>::load(dp + ca + dg_, dg);
#pragma unroll
      for (int e = 0; e < CH; ++e) o[e] = da[e] * av[e] + dg[e] * gv[e];          // av = G1, gv = G2
      Vec<T>::store((T*)a.y + row * a.F + c, o);
    } else {
      float gy[CH], o2[CH];
      Vec<T>::load((const T*)a.d + row * a.F + c, gy);
#pragma unroll
      for (int e = 0; e < CH; ++e) {
        o[e] = gy[e] * av[e];
        o2[e] = gy[e] * gv[e];
      }
      T* yp = (T*)a.y + row * 2 * a.F;
      if (a.accumulate) {
        float t1[CH], t2[CH];
        Vec<T>::load(yp + ca, t1);
        Vec<T>::load(yp + ca + dg_, t2);
#pragma unroll
        for (int e = 0; e < CH; ++e) { o[e] += t1[e]; o2[e] += t2[e]; }
      }
      Vec<T>::store(yp + ca, o);
      Vec<T>::store(yp + ca + dg_, o2);
    }
  }
}

template <typename T>
static int geglu_t(int mode, const GegluArgs& a, hipStream_t st) {
  if (a.F % TT<T>::CH) { set_error("geglu: F=%d not chunk aligned", a.F); return -1; }
  if (a.il && (a.il != 64 || a.F % 64)) { set_error("geglu: interleave %d with F=%d unsupported (blocks of 64)", a.il, a.F); return -1; }
  long nrows = (long)(mode == MODE_PRIMAL ? a.Bp : a.NT) * a.rows_per_sample;
  unsigned g = grid_for(nrows * (a.F / TT<T>::CH));
  if (mode == MODE_PRIMAL) DPB_LAUNCH((geglu_kernel<T, MODE_PRIMAL>), dim3(g), dim3(256), 0, st, a, nrows);
  else if (mode == MODE_TANGENT) DPB_LAUNCH((geglu_kernel<T, MODE_TANGENT>), dim3(g), dim3(256), 0, st, a, nrows);
  else DPB_LAUNCH((geglu_kernel<T, MODE_ADJOINT>), dim3(g), dim3(256), 0, st, a, nrows);
  DPB_CHECK(hipGetLastError());
  return 0;
}
int launch_geglu(int dtype, int mode, const GegluArgs& a, hipStream_t st) {
  return DPB_DISPATCH_T(dtype, T, geglu_t<T>(mode, a, st));
}

template <typename T, int OP>   // 0: silu  1: y = x  2: y += x  3: quick_gelu  4: exact (erf) gelu
__global__ __launch_bounds__(256) void unary_kernel(const T* x, T* y, long nchunks) {
  constexpr int CH = TT<T>::CH;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nchunks; i += (long)gridDim.x * 256) {
    float v[CH];
    Vec<T>::load(x + i * CH, v);
    if (OP == 0) {
#pragma unroll
      for (int e = 0; e < CH; ++e) v[e] = silu_(v[e]);
    } else if (OP == 3) {
#pragma unroll
      for (int e = 0; e < CH; ++e) v[e] = v[e] / (1.f + __expf(-1.702f * v[e]));
    } else if (OP == 4) {
#pragma unroll
      for (int e = 0; e < CH; ++e) v[e] = gelu_(v[e]);
    } else if (OP == 2) {
      float o[CH];
      Vec<T>::load(y + i * CH, o);
#pragma unroll
      for (int e = 0; e < CH; ++e) v[e] += o[e];
    }
    Vec<T>::store(y + i * CH, v);
  }
}

template <typename T>
static int unary_t(int op, const void* x, void* y, long n, hipStream_t st) {
  if (n % TT<T>::CH) { set_error("elementwise: n=%ld not chunk aligned", n); return -1; }
  long nc = n / TT<T>::CH;
  unsigned g = grid_for(nc);
  if (op == 0) DPB_LAUNCH((unary_kernel<T, 0>), dim3(g), dim3(256), 0, st, (const T*)x, (T*)y, nc);
  else if (op == 1) DPB_LAUNCH((unary_kernel<T, 1>), dim3(g), dim3(256), 0, st, (const T*)x, (T*)y, nc);
  else if (op == 3) DPB_LAUNCH((unary_kernel<T, 3>), dim3(g), dim3(256), 0, st, (const T*)x, (T*)y, nc);
  else if (op == 4) DPB_LAUNCH((unary_kernel<T, 4>), dim3(g), dim3(256), 0, st, (const T*)x, (T*)y, nc);
  else DPB_LAUNCH((unary_kernel<T, 2>), dim3(g), dim3(256), 0, st, (const T*)x, (T*)y, nc);
  DPB_CHECK(hipGetLastError());
  return 0;
}
int launch_silu(int dtype, const void* x, void* y, long n, hipStream_t st) {
  return DPB_DISPATCH_T(dtype, T, unary_t<T>(0, x, y, n, st));
}
int launch_quick_gelu(int dtype, const void* x, void* y, long n, hipStream_t st) {
  return DPB_DISPATCH_T(dtype, T, unary_t<T>(3, x, y, n, st));
}
int launch_gelu(int dtype, const void* x, void* y, long n, hipStream_t st) {
  return DPB_DISPATCH_T(dtype, T, unary_t<T>(4, x, y, n, st));
}

// token + position embedding lookup of the text encoder, written in the engine's fp32 [b][c][t] boundary layout
template <typename T>
__global__ __launch_bounds__(256) void embed_tokens_kernel(const int* ids, const T* tok, const T* pos, float* out, int L, int C, int vocab) {
  const int b = blockIdx.y, t = blockIdx.x;
  int id = ids[b * L + t];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  for (int c = threadIdx.x; c < C; c += 256)
    out[((long)b * C + c) * L + t] = TT<T>::ld(tok + (long)id * C + c) + TT<T>::ld(pos + (long)t * C + c);
}
int launch_embed_tokens(int dtype, const int* ids, const void* tok, const void* pos, float* out, int batch, int L, int C, int vocab, hipStream_t st) {
  if (batch <= 0 || L <= 0 || C <= 0 || vocab <= 0) { set_error("embed_tokens: empty problem"); return -1; }
  DPB_DISPATCH_STMT(dtype, T, DPB_LAUNCH((embed_tokens_kernel<T>), dim3(L, batch), dim3(256), 0, st, ids, (const T*)tok, (const T*)pos, out, L, C, vocab));
  DPB_CHECK(hipGetLastError());
  return 0;
}

int launch_axpy(int dtype, const void* x, void* y, long n, int accumulate, hipStream_t st) {
  int op = accumulate ? 2 : 1;
  return DPB_DISPATCH_T(dtype, T, unary_t<T>(op, x, y, n, st));
}

template <typename T>
__global__ __launch_bounds__(256) void copy_cols_kernel(const T* src, int lds_, int cs0, T* dst, int ldd, int cd0, long rows,
                                                        int ncols, int accumulate) {
  constexpr int CH = TT<T>::CH;
  const int nch = ncols / CH;
  const long total = rows * nch;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long r = idx / nch;
    const int c = (int)(idx - r * nch) * CH;
    float v[CH];
    Vec<T>::load(src + r * lds_ + cs0 + c, v);
    T* dp = dst + r * ldd + cd0 + c;
    if (accumulate) {
      float o[CH];
      Vec<T>::load(dp, o);
#pragma unroll
      for (int e = 0; e < CH; ++e) v[e] += o[e];
    }
    Vec<T>::store(dp, v);
  }
}
int launch_copy_cols(int dtype, const void* src, int lds_, int cs0, void* dst, int ldd, int cd0, long rows, int ncols, int accumulate,
                     hipStream_t st) {
  int CH = dt_chunk(dtype);
  if (ncols % CH || cs0 % CH || cd0 % CH || lds_ % CH || ldd % CH) { set_error("copy_cols: misaligned window"); return -1; }
  unsigned g = grid_for(rows * (ncols / CH));
  DPB_DISPATCH_STMT(dtype, T, DPB_LAUNCH((copy_cols_kernel<T>), dim3(g), dim3(256), 0, st, (const T*)src, lds_, cs0, (T*)dst, ldd, cd0, rows, ncols, accumulate));
  DPB_CHECK(hipGetLastError());
  return 0;
}

// zero a column window dst[r][cd0 .. cd0+ncols) of a [rows][ldd] tensor (tangent of the inactive operand of a concat: the window may hold a
// pass of another seed; the rest of the tensor is written by the concat's other copy)
template <typename T>
__global__ __launch_bounds__(256) void zero_cols_kernel(T* dst, int ldd, int cd0, long rows, int ncols) {
  constexpr int CH = TT<T>::CH;
  const int nch = ncols / CH;
  const long total = rows * nch;
  float v[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) v[e] = 0.f;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long r = idx / nch;
    const int c = (int)(idx - r * nch) * CH;
    Vec<T>::store(dst + r * ldd + cd0 + c, v);
  }
}
int launch_zero_cols(int dtype, void* dst, int ldd, int cd0, long rows, int ncols, hipStream_t st) {
  int CH = dt_chunk(dtype);
  if (ncols % CH || cd0 % CH || ldd % CH || cd0 + ncols > ldd) { set_error("zero_cols: misaligned window"); return -1; }
  unsigned g = grid_for(rows * (ncols / CH));
  DPB_DISPATCH_STMT(dtype, T, DPB_LAUNCH((zero_cols_kernel<T>), dim3(g), dim3(256), 0, st, (T*)dst, ldd, cd0, rows, ncols));
  DPB_CHECK(hipGetLastError());
  return 0;
}

// fp32 NCHW -> T NHWC (channel pad to Cpad with zeros).  Small tensors (boundary only): tile transpose through LDS.
template <typename T>
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float* src, T* dst, int C, int HW, int Cpad) {
  __shared__ float tile[32][33];
  const int n = blockIdx.z;
  const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int k = ty; k < 32; k += 8) {   // k: channel, tx: pixel (contiguous in src)
    int c = c0 + k, p = p0 + tx;
    tile[k][tx] = (c < C && p < HW) ? src[((long)n * C + c) * HW + p] : 0.f;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {   // k: pixel, tx: channel (contiguous in dst)
    int p = p0 + k, c = c0 + tx;
    if (p < HW && c < Cpad) TT<T>::st(dst + ((long)n * HW + p) * Cpad + c, tile[tx][k]);
  }
}
template <typename T>
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const T* src, float* dst, int C, int HW, int Cpad) {
  __shared__ float tile[32][33];
  const int n = blockIdx.z;
  const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int k = ty; k < 32; k += 8) {   // k: pixel, tx: channel
    int p = p0 + k, c = c0 + tx;
    tile[k][tx] = (p < HW && c < C) ? TT<T>::ld(src + ((long)n * HW + p) * Cpad + c) : 0.f;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {   // k: channel, tx: pixel
    int c = c0 + k, p = p0 + tx;
    if (c < C && p < HW) dst[((long)n * C + c) * HW + p] = tile[tx][k];
  }
}
int launch_nchw_to_nhwc(int dtype, const float* src, void* dst, int n, int C, int HW, int Cpad, hipStream_t st) {
  dim3 grid((HW + 31) / 32, (Cpad + 31) / 32, n);
  DPB_DISPATCH_STMT(dtype, T, DPB_LAUNCH((nchw_to_nhwc_kernel<T>), grid, dim3(256), 0, st, src, (T*)dst, C, HW, Cpad));
  DPB_CHECK(hipGetLastError());
  return 0;
}
int launch_nhwc_to_nchw(int dtype, const void* src, float* dst, int n, int C, int HW, int Cpad, hipStream_t st) {
  dim3 grid((HW + 31) / 32, (C + 31) / 32, n);
  DPB_DISPATCH_STMT(dtype, T, DPB_LAUNCH((nhwc_to_nchw_kernel<T>), grid, dim3(256), 0, st, (const T*)src, dst, C, HW, Cpad));
  DPB_CHECK(hipGetLastError());
  return 0;
}

// h-space shift of a tap, the seam of dpb_forward_shift and dpb_forward_shift_groups: h holds the xb samples the prefix computed (rows 0 .. xb-1 of
// [groups xb][HW][C]); row g xb + b becomes h[b] + scale u[dir] for every group g.  (xb, groups) = (1, batch): every row is a shifted copy of sample 0;
// (batch, 1): every row is shifted in place.  h: the tap, NHWC in T (C - Cv pad channels, copied); u: fp32 [nu][Cv][HW], the NCHW-flattened layout of
// every tap at the boundary.  One block owns a tile of 32 pixels x 64 channels for ALL rows: sample b's tile is read into registers before any of its
// copies is written, and no other row is a source, so the in-place write of group 0 has no hazard.  u goes through LDS (read along pixels, written
// along channels); the sum is formed in fp32 and rounded once by the store.  VEC: elements per access on the NHWC side (a 16-byte chunk, or 1).
// rows: the (dir, scale) of samples b0 .. b0 + nb - 1 in groups g0 .. g0 + ng - 1, entry g nb + r for group g0 + g; a row of group 0 with dir < 0 is
// its own source and is left alone, every other row is written.
constexpr int SHIFT_TP = 32, SHIFT_TC = 64;
template <typename T, int VEC>
__global__ __launch_bounds__(256) void shift_tap_kernel(T* h, const float* u, ShiftRows rows, int b0, int nb, int g0, int ng, int xb, int C, int Cv,
                                                        long HW) {
  constexpr int CPP = SHIFT_TC / VEC;                    // accesses per pixel of the tile
  constexpr int ITER = SHIFT_TP * CPP / 256;
  __shared__ float tile[SHIFT_TC][SHIFT_TP + 1];
  const long p0 = (long)blockIdx.x * SHIFT_TP;
  const int c0 = blockIdx.y * SHIFT_TC;
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
    for (int g = 0; g < ng; ++g) {
      const int dir = rows.dir[g * nb + r];
      const float sc = rows.scale[g * nb + r];
      if (dir < 0 && g0 + g == 0) continue;                // unshifted row that is its own source: nothing to write (uniform over the block)
      if (dir >= 0) {
        __syncthreads();                                   // the tile of the row before has been read
        const float* ub = u + (long)dir * Cv * HW;
        for (int k = ty; k < SHIFT_TC; k += 8) {
          const int c = c0 + k;
          tile[k][tx] = (c < Cv && p0 + tx < HW) ? ub[(long)c * HW + p0 + tx] : 0.f;
        }
        __syncthreads();
      }
      T* hb = h + ((long)(g0 + g) * xb + b) * img;
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
static int shift_tap_t(void* h, const float* u, const int* dir, const float* scale, int xb, int groups, int C, int Cv, long HW, hipStream_t st) {
  const dim3 grid((unsigned)((HW + SHIFT_TP - 1) / SHIFT_TP), (unsigned)((C + SHIFT_TC - 1) / SHIFT_TC));
  // rows travel as kernel arguments, SHIFT_MAX_ROWS per launch: every group of as many samples as fit, or -- more groups than that -- one sample's
  // groups in chunks, the chunk holding group 0 (the source of the others) last
  const int gper = std::min(groups, SHIFT_MAX_ROWS), per = SHIFT_MAX_ROWS / gper;
  for (int g0 = (groups - 1) / gper * gper; g0 >= 0; g0 -= gper)
    for (int b0 = 0; b0 < xb; b0 += per) {
      ShiftRows rows;
      const int ng = std::min(gper, groups - g0), nb = std::min(per, xb - b0);
      for (int g = 0; g < ng; ++g)
        for (int r = 0; r < nb; ++r) { rows.dir[g * nb + r] = dir[(g0 + g) * xb + b0 + r]; rows.scale[g * nb + r] = scale[(g0 + g) * xb + b0 + r]; }
      if (C % TT<T>::CH == 0) DPB_LAUNCH((shift_tap_kernel<T, TT<T>::CH>), grid, dim3(256), 0, st, (T*)h, u, rows, b0, nb, g0, ng, xb, C, Cv, HW);
      else DPB_LAUNCH((shift_tap_kernel<T, 1>), grid, dim3(256), 0, st, (T*)h, u, rows, b0, nb, g0, ng, xb, C, Cv, HW);
      DPB_CHECK(hipGetLastError());
    }
  return 0;
}
int launch_shift_tap(int dtype, void* h, const float* u, const int* dir, const float* scale, int xb, int groups, int C, int Cv, long HW,
                     hipStream_t st) {
  if (xb < 1 || groups < 1 || C < 1 || Cv < 1 || Cv > C || HW < 1) { set_error("shift_tap: empty or inconsistent problem"); return -1; }
  return DPB_DISPATCH_T(dtype, T, shift_tap_t<T>(h, u, dir, scale, xb, groups, C, Cv, HW, st));
}

// sample 0 of every buffer of a descriptor table -> samples 1 .. batch-1, in place, 16-byte copies (blockIdx.y: the buffer)
__global__ __launch_bounds__(256) void replicate_rows_kernel(ReplTable t, int batch) {
  uint4* p = (uint4*)t.p[blockIdx.y];
  const long n = t.chunks[blockIdx.y];
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const uint4 v = p[i];
    for (int b = 1; b < batch; ++b) p[(long)b * n + i] = v;
  }
}
int launch_replicate_rows(void* const* bufs, const size_t* sample_bytes, int nbufs, int batch, hipStream_t st) {
  if (batch < 2) return 0;
  for (int i0 = 0; i0 < nbufs; i0 += REPL_MAX_BUFS) {
    ReplTable t;
    const int n = std::min(REPL_MAX_BUFS, nbufs - i0);
    long most = 1;
    for (int i = 0; i < n; ++i) {
      if (sample_bytes[i0 + i] % 16 || (uintptr_t)bufs[i0 + i] % 16) { set_error("replicate_rows: buffer %d is not a whole number of aligned 16-byte chunks per sample", i0 + i); return -1; }
      t.p[i] = bufs[i0 + i];
      t.chunks[i] = (long)(sample_bytes[i0 + i] / 16);
      most = std::max(most, t.chunks[i]);
    }
    DPB_LAUNCH(replicate_rows_kernel, dim3(std::min(grid_for(most), 2048u), n), dim3(256), 0, st, t, batch);
    DPB_CHECK(hipGetLastError());
  }
  return 0;
}

template <typename T>
__global__ __launch_bounds__(256) void pool2x2_kernel(const T* in, T* out, int n, int H, int W, int C, int accumulate, float scale) {
  constexpr int CH = TT<T>::CH;
  const int cch = C / CH;
  const long total = (long)n * H * W * cch;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int c = (int)(idx % cch) * CH;
    long pix = idx / cch;
    const int x = (int)(pix % W);
    pix /= W;
    const int y = (int)(pix % H);
    const long s = pix / H;
    float acc[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) acc[e] = 0.f;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        float v[CH];
        Vec<T>::load(in + ((s * 2 * H + 2 * y + dy) * 2 * W + 2 * x + dx) * C + c, v);
#pragma unroll
        for (int e = 0; e < CH; ++e) acc[e] += v[e];
      }
    T* op = out + ((s * H + y) * W + x) * C + c;
#pragma unroll
    for (int e = 0; e < CH; ++e) acc[e] *= scale;            // (1: the sum itself, bit for bit)
    if (accumulate) {
      float o[CH];
      Vec<T>::load(op, o);
#pragma unroll
      for (int e = 0; e < CH; ++e) acc[e] += o[e];
    }
    Vec<T>::store(op, acc);
  }
}
// out[s][Y][X][c] (+)= scale * in[s][Y / 2][X / 2][c] on the 2H x 2W grid: nearest x2 upsampling (scale 1) and the adjoint of the 2x2 average
// pool (scale 0.25).  One thread per 16-byte chunk of the OUTPUT (coalesced stores; each input chunk is read by four threads, from L2).
template <typename T>
__global__ __launch_bounds__(256) void up2x2_kernel(const T* in, T* out, int n, int H, int W, int C, int accumulate, float scale) {
  constexpr int CH = TT<T>::CH;
  const int cch = C / CH;
  const long total = (long)n * 4 * H * W * cch;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int c = (int)(idx % cch) * CH;
    long pix = idx / cch;
    const int X = (int)(pix % (2 * W));
    pix /= 2 * W;
    const int Y = (int)(pix % (2 * H));
    const long s = pix / (2 * H);
    float v[CH];
    Vec<T>::load(in + ((s * H + (Y >> 1)) * W + (X >> 1)) * C + c, v);
#pragma unroll
    for (int e = 0; e < CH; ++e) v[e] *= scale;
    T* op = out + ((s * 2 * H + Y) * 2 * W + X) * C + c;
    if (accumulate) {
      float o[CH];
      Vec<T>::load(op, o);
#pragma unroll
      for (int e = 0; e < CH; ++e) v[e] += o[e];
    }
    Vec<T>::store(op, v);
  }
}
static int resample_check(const char* what, int dtype, const void* in, const void* out, int n, int H, int W, int C) {
  if (!in || !out || n < 1 || H < 1 || W < 1 || C < 1 || C % dt_chunk(dtype)) {
    set_error("%s: n=%d H=%d W=%d C=%d (C must be a positive multiple of the 16-byte chunk)", what, n, H, W, C);
    return -1;
  }
  return 0;
}
int launch_pool2x2(int dtype, const void* in, void* out, int n, int H, int W, int C, float scale, int accumulate, hipStream_t st) {
  if (resample_check("pool2x2", dtype, in, out, n, H, W, C)) return -1;
  unsigned g = grid_for((long)n * H * W * (C / dt_chunk(dtype)));
  DPB_DISPATCH_STMT(dtype, T, DPB_LAUNCH((pool2x2_kernel<T>), dim3(g), dim3(256), 0, st, (const T*)in, (T*)out, n, H, W, C, accumulate, scale));
  DPB_CHECK(hipGetLastError());
  return 0;
}
int launch_up2x2(int dtype, const void* in, void* out, int n, int H, int W, int C, float scale, int accumulate, hipStream_t st) {
  if (resample_check("up2x2", dtype, in, out, n, H, W, C)) return -1;
  unsigned g = grid_for((long)n * 4 * H * W * (C / dt_chunk(dtype)));
  DPB_DISPATCH_STMT(dtype, T, DPB_LAUNCH((up2x2_kernel<T>), dim3(g), dim3(256), 0, st, (const T*)in, (T*)out, n, H, W, C, accumulate, scale));
  DPB_CHECK(hipGetLastError());
  return 0;
}
int launch_pool2x2_sum(int dtype, const void* in, void* out, int n, int H, int W, int C, int accumulate, hipStream_t st) {
  int CH = dt_chunk(dtype);
  unsigned g = grid_for((long)n * H * W * (C / CH));
  DPB_DISPATCH_STMT(dtype, T, DPB_LAUNCH((pool2x2_kernel<T>), dim3(g), dim3(256), 0, st, (const T*)in, (T*)out, n, H, W, C, accumulate, 1.f));
  DPB_CHECK(hipGetLastError());
  return 0;
}

__global__ __launch_bounds__(256) void ddim_kernel(const float* x, const float* e, float* out, float* x0, long n, float sa, float s1a,
                                                   float san, float s1an) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    float p = (x[i] - e[i] * s1a) / sa;
    if (x0) x0[i] = p;
    out[i] = san * p + s1an * e[i];
  }
}
int launch_ddim_step(const float* x, const float* e, float* out, float* x0, long n, float a_t, float a_next, hipStream_t st) {
  // same operation order as the reference (utils.py:301-306): sqrt in fp32 of the fp32 alphas
  DPB_LAUNCH(ddim_kernel, dim3(grid_for(n)), dim3(256), 0, st, x, e, out, x0, n, sqrtf(a_t), sqrtf(1.f - a_t), sqrtf(a_next),
                     sqrtf(1.f - a_next));
  DPB_CHECK(hipGetLastError());
  return 0;
}

__global__ __launch_bounds__(256) void lincomb_kernel(const float* x, const float* y, const float* z, float* out, long n, float a, float b,
                                                      float c) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    float v = a * x[i] + b * y[i];
    if (z) v += c * z[i];
    out[i] = v;
  }
}
int launch_lincomb(const float* x, const float* y, const float* z, float* out, long n, float a, float b, float c, hipStream_t st) {
  DPB_LAUNCH(lincomb_kernel, dim3(grid_for(n)), dim3(256), 0, st, x, y, z, out, n, a, b, c);
  DPB_CHECK(hipGetLastError());
  return 0;
}

}  // namespace dpb
