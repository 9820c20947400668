// The parallel-h edit chain (reference src/modules/edit.py:1202-1229, :1470-1497): the h-space direction c is held fixed and the x-space direction is
// recomputed at every state, v = -J^T c / ||J^T c|| (PullBackDDPM.inv_jac_xt, src/models/ddpm/diffusion.py:347-377), x <- x + step v, optionally
// with the SEGA rule v <- where(|v| < sigma std(v), 0, v).  The U-Net passes are the engine's; this file holds what lies between them:
//   direction step   W = J^T c [n][N] -> v, the SEGA mask, x_out = x + step v and the per-row statistics (S2, std, kept, flag);
//   shift statistics a = <h - h0, c> / ||c|| and q = ||h - h0||^2 per row, c = sign u[dir];
//   cotangent gather cot[b] = sign[b] u[dir[b]].
// fp32 in / fp32 out, every sum in fp64 in ONE fixed chain: thread t of a workgroup adds the elements of its groups of four in index order into its own
// accumulator, the 256 accumulators meet in block_sum, and a row's slices of ROW_SLICE elements are added in slice order by every workgroup that needs
// the total.  No atomics in any floating-point sum: a row's results are a function of the row and N only -- not of n, of the row's position in the
// stack or of the alignment of its pointers (the 16-byte and the 4-byte access paths give every thread the same elements in the same order).  The
// count of kept elements is a sum of integers below 2^53, exact in fp64 in any order: the workgroups add theirs with one fp64 atomic each.
// Rows start at b N floats, so a row is 16-byte aligned only when b N % 4 == 0: each workgroup tests the row pointers it touches and takes the
// 16-byte path for the whole groups of an aligned row, the 4-byte path otherwise and for the ragged last group.
#include "kernels.h"
#include "geom.h"

namespace dpb {

namespace {

struct ChainSteps { float v[CHAIN_MAX_ROWS]; };               // host lists travel as kernel arguments, CHAIN_MAX_ROWS rows per launch
struct ChainDirs { int dir[CHAIN_MAX_ROWS]; float sign[CHAIN_MAX_ROWS]; };

// part[b][slice] = (sum w, sum w^2) of the slice in fp64; the workgroup of slice 0 clears the row's kept count (stats[b][2]) for the apply kernel
__global__ __launch_bounds__(ROW_NT) void chain_partial_kernel(const float* W, long N, double* part, double* stats) {
  __shared__ double red[ROW_NT / 64];
  const int b = blockIdx.y, t = threadIdx.x;
  const long nsl = gridDim.x;
  const float* row = W + (long)b * N;
  const bool al = aligned16(row);
  double s1 = 0.0, s2 = 0.0;
#pragma unroll
  for (int i = 0; i < ROW_GROUPS; ++i) {
    const long j = (long)blockIdx.x * ROW_SLICE + ((long)i * ROW_NT + t) * 4;
    if (j < N) {
      const float4 w = row_load4(row, j, N, al);
      const double a0 = w.x, a1 = w.y, a2 = w.z, a3 = w.w;
      s1 += a0; s1 += a1; s1 += a2; s1 += a3;
      s2 += a0 * a0; s2 += a1 * a1; s2 += a2 * a2; s2 += a3 * a3;
    }
  }
  s1 = block_sum<ROW_NT>(s1, red);
  s2 = block_sum<ROW_NT>(s2, red);
  if (t == 0) {
    double* p = part + ((long)b * nsl + blockIdx.x) * 2;
    p[0] = s1; p[1] = s2;
    if (blockIdx.x == 0) stats[(long)b * 4 + 2] = 0.0;
  }
}

// v = fl32(-w / sqrt(S2)), the SEGA mask, x_out = fl32(x + step v); the workgroup of slice 0 writes the row's (S2, std, . , flag)
__global__ __launch_bounds__(ROW_NT) void chain_apply_kernel(const float* W, const float* x, float* x_out, float* vk, long N, ChainSteps steps,
                                                            double sega_sigma, const double* part, double* stats) {
  __shared__ double red[ROW_NT / 64];
  __shared__ double row_s[2];
  const int b = blockIdx.y, t = threadIdx.x;
  const long nsl = gridDim.x, off = (long)b * N;
  if (t == 0) sum_slices<2>(part + (long)b * nsl * 2, nsl, row_s);
  __syncthreads();
  const double S1 = row_s[0], S2 = row_s[1];
  const bool bad = !(S2 > 0.0) || !(S2 < 1.7e308);          // zero, NaN or inf: the row has no direction
  const double rn = sqrt(S2);
  const bool sega = sega_sigma > 0.0 && N >= 2 && !bad;
  double sd = 0.0;
  if (sega) {
    const double var = (1.0 - S1 * S1 / ((double)N * S2)) / (double)(N - 1);   // unbiased variance of the unit-norm row, in the two sums
    sd = sqrt(var > 0.0 ? var : 0.0);
  }
  const double thr = sega_sigma * sd, step = (double)steps.v[b];
  const float nanf_ = __builtin_nanf("");
  const bool alw = aligned16(W + off), alx = aligned16(x + off), alo = aligned16(x_out + off), alv = vk && aligned16(vk + off);
  double kept = 0.0;
#pragma unroll
  for (int i = 0; i < ROW_GROUPS; ++i) {
    const long j = (long)blockIdx.x * ROW_SLICE + ((long)i * ROW_NT + t) * 4;
    if (j >= N) continue;
    const float4 w = row_load4(W + off, j, N, alw);
    const float4 xv = row_load4(x + off, j, N, alx);
    const float wi[4] = {w.x, w.y, w.z, w.w}, xi[4] = {xv.x, xv.y, xv.z, xv.w};
    float vo[4], xo[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float v = (float)(-(double)wi[c] / rn);
      const bool cut = sega && fabs((double)v) < thr;
      if (cut) v = 0.f;
      if (j + c < N && !cut) kept += 1.0;
      vo[c] = bad ? nanf_ : v;
      xo[c] = bad ? nanf_ : (float)((double)xi[c] + step * (double)v);
    }
    row_store4(x_out + off, j, N, alo, make_float4(xo[0], xo[1], xo[2], xo[3]));
    if (vk) row_store4(vk + off, j, N, alv, make_float4(vo[0], vo[1], vo[2], vo[3]));
  }
  kept = block_sum<ROW_NT>(bad ? 0.0 : kept, red);
  if (t == 0) {
    double* st = stats + (long)b * 4;
    if (kept != 0.0) atomicAdd(st + 2, kept);              // integers below 2^53: exact, the order of the workgroups does not matter
    if (blockIdx.x == 0) { st[0] = S2; st[1] = sd; st[3] = bad ? 1.0 : 0.0; }
  }
}

// out[b] = (a, q): a = <h - h0, c> / ||c||, q = ||h - h0||^2, c = sign[b] u[dir[b]]; one workgroup per row, the chain of rowsumsq_kernel
__global__ __launch_bounds__(ROW_NT) void chain_shift_kernel(const float* h, const float* h0, const float* u, long D, ChainDirs dirs, double* out) {
  __shared__ double red[ROW_NT / 64];
  const int b = blockIdx.x;
  const float *hr = h + (long)b * D, *gr = h0 + (long)b * D, *ur = u + (long)dirs.dir[b] * D;
  const bool alh = aligned16(hr), alg = aligned16(gr), alu = aligned16(ur);
  const double sg = (double)dirs.sign[b];
  double dc = 0.0, cc = 0.0, dd = 0.0;
  for (long j = (long)threadIdx.x * 4; j < D; j += ROW_NT * 4) {
    const float4 a = row_load4(hr, j, D, alh), g = row_load4(gr, j, D, alg), c4 = row_load4(ur, j, D, alu);
    const double d[4] = {(double)a.x - (double)g.x, (double)a.y - (double)g.y, (double)a.z - (double)g.z, (double)a.w - (double)g.w};
    const double c[4] = {sg * (double)c4.x, sg * (double)c4.y, sg * (double)c4.z, sg * (double)c4.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { dc += d[i] * c[i]; cc += c[i] * c[i]; dd += d[i] * d[i]; }
  }
  dc = block_sum<ROW_NT>(dc, red);
  cc = block_sum<ROW_NT>(cc, red);
  dd = block_sum<ROW_NT>(dd, red);
  if (threadIdx.x == 0) { out[(long)b * 2] = dc / sqrt(cc); out[(long)b * 2 + 1] = dd; }
}

// cot[b][j] = sign[b] * u[dir[b]][j] (one fp32 product: exact for sign = +-1)
__global__ __launch_bounds__(ROW_NT) void chain_gather_kernel(const float* u, long D, ChainDirs dirs, float* cot) {
  const int b = blockIdx.y;
  const long j = ((long)blockIdx.x * ROW_NT + threadIdx.x) * 4;
  if (j >= D) return;
  const float* ur = u + (long)dirs.dir[b] * D;
  float* cr = cot + (long)b * D;
  float4 v = row_load4(ur, j, D, aligned16(ur));
  const float s = dirs.sign[b];
  v.x *= s; v.y *= s; v.z *= s; v.w *= s;
  row_store4(cr, j, D, aligned16(cr), v);
}

int fill_dirs(const char* who, ChainDirs& d, const int32_t* dir, const float* sign, long r0, int rows, int nu) {
  for (int i = 0; i < rows; ++i) {
    if (dir[r0 + i] < 0 || dir[r0 + i] >= nu) { set_error("%s: dir[%ld]=%d outside [0,%d)", who, r0 + i, dir[r0 + i], nu); return -1; }
    if (!std::isfinite(sign[r0 + i])) { set_error("%s: sign[%ld] is not finite", who, r0 + i); return -1; }
    d.dir[i] = dir[r0 + i]; d.sign[i] = sign[r0 + i];
  }
  return 0;
}

}  // namespace

size_t direction_step_scratch_bytes(long n, long N) { return row_partial_bytes(n, N); }

int launch_direction_step(const float* W, const float* x, float* x_out, float* vk, const float* step, float sega_sigma, long n, long N, double* stats,
                          void* scratch, size_t scratch_bytes, hipStream_t st) {
  if (check_rows("direction_step", n, N)) return -1;
  if (scratch_bytes < direction_step_scratch_bytes(n, N)) {
    set_error("direction_step: scratch of %zu bytes, dpb_direction_step_scratch_bytes(%ld, %ld) = %zu", scratch_bytes, n, N, direction_step_scratch_bytes(n, N));
    return -1;
  }
  if ((uintptr_t)scratch & 7 || (uintptr_t)stats & 7) { set_error("direction_step: scratch and stats must be 8-byte aligned"); return -1; }
  if (std::isnan(sega_sigma)) { set_error("direction_step: sega_sigma is NaN"); return -1; }
  for (long b = 0; b < n; ++b)
    if (!std::isfinite(step[b])) { set_error("direction_step: step[%ld] is not finite", b); return -1; }
  const long nsl = row_slices(N);
  double* part = (double*)scratch;
  for (long r0 = 0; r0 < n; r0 += CHAIN_MAX_ROWS) {
    const int rows = (int)std::min<long>(CHAIN_MAX_ROWS, n - r0);
    ChainSteps s;
    for (int i = 0; i < rows; ++i) s.v[i] = step[r0 + i];
    const dim3 grid((unsigned)nsl, (unsigned)rows), block(ROW_NT);
    const long o = r0 * N;
    DPB_LAUNCH(chain_partial_kernel, grid, block, 0, st, W + o, N, part + r0 * nsl * 2, stats + r0 * 4);
    DPB_LAUNCH(chain_apply_kernel, grid, block, 0, st, W + o, x + o, x_out + o, vk ? vk + o : nullptr, N, s, (double)sega_sigma,
               (const double*)(part + r0 * nsl * 2), stats + r0 * 4);
  }
  DPB_CHECK(hipGetLastError());
  return 0;
}

int launch_shift_stats(const float* h, const float* h0, const float* u, int nu, const int32_t* dir, const float* sign, long n, long D, double* out,
                       hipStream_t st) {
  if (check_rows("shift_stats", n, D)) return -1;
  if (nu < 1) { set_error("shift_stats: nu=%d: at least one direction is needed", nu); return -1; }
  if ((uintptr_t)out & 7) { set_error("shift_stats: out must be 8-byte aligned"); return -1; }
  for (long r0 = 0; r0 < n; r0 += CHAIN_MAX_ROWS) {
    const int rows = (int)std::min<long>(CHAIN_MAX_ROWS, n - r0);
    ChainDirs d;
    if (fill_dirs("shift_stats", d, dir, sign, r0, rows, nu)) return -1;
    DPB_LAUNCH(chain_shift_kernel, dim3((unsigned)rows), dim3(ROW_NT), 0, st, h + r0 * D, h0 + r0 * D, u, D, d, out + r0 * 2);
  }
  DPB_CHECK(hipGetLastError());
  return 0;
}

int launch_gather_cotangents(const float* u, int nu, const int32_t* dir, const float* sign, long n, long D, float* cot, hipStream_t st) {
  if (check_rows("gather_cotangents", n, D)) return -1;
  if (nu < 1) { set_error("gather_cotangents: nu=%d: at least one direction is needed", nu); return -1; }
  const long ng = (D + 3) / 4;
  for (long r0 = 0; r0 < n; r0 += CHAIN_MAX_ROWS) {
    const int rows = (int)std::min<long>(CHAIN_MAX_ROWS, n - r0);
    ChainDirs d;
    if (fill_dirs("gather_cotangents", d, dir, sign, r0, rows, nu)) return -1;
    DPB_LAUNCH(chain_gather_kernel, dim3((unsigned)((ng + ROW_NT - 1) / ROW_NT), (unsigned)rows), dim3(ROW_NT), 0, st, u, D, d, cot + r0 * D);
  }
  DPB_CHECK(hipGetLastError());
  return 0;
}

}  // namespace dpb
