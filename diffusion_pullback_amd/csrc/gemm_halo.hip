// bf16 3x3 stride-1 convolution (forward gather and its adjoint), halo-tile form of the LDS-ring MFMA GEMM.
//
// gemm_ring64.hip runs a 3x3 convolution as an implicit GEMM: every K-step DMAs a fresh [pixels][64 channels] A tile, so
// each input pixel travels L2 -> LDS nine times (once per filter tap), and the measured limiter of that kernel is exactly
// this DMA stream (profiles/r01_gemm_ablation.txt).  Here a block owns 256 output pixels = R whole image rows of one
// sample and keeps the (R+2) x (W+2) pixel HALO of one 64-channel chunk in LDS; the nine taps of that chunk read their A
// fragments from it at shifted pixel offsets, and only the [128 x 64] weight tile streams per K-step:
//   bytes through the DMA per 256x128 output tile and 64-channel chunk:  ~50 KB halo + 9 x 16 KB weights = 194 KB
//   versus 9 x (32 + 16) KB = 432 KB for the implicit-GEMM form of the same tile (0.45x; 0.34x of two 128x128 tiles).
// 8 waves (4 x 2, 64x64 wave tiles) so that one resident block still gives every SIMD two waves; LDS = 2 halo buffers
// (the next chunk's halo lands while the current one is consumed) + the weight ring: 3 stages of 16 KiB in the ring loop, 6 half-tile
// slots of 8 KiB in the 8-phase loop (149 KiB either way).
//
// K order is chunk-major (chunk, then tap), so results differ from the tap-major kernels in fp32 association only.
// Halo pixel p of a buffer lives at p*128 B, chunk c at ((c ^ ((p >> 1) & 7)) * 16 B (same source-side swizzle as the
// ring: conflict-free ds_read_b128 for runs of consecutive pixels); out-of-image pixels read the zero page.
// Two main loops over the same tile, LDS image and K order (bitwise equal results): the 8-phase loop (halo_p8_loop, default: two wave groups one
// barrier apart, counted vmcnt waits, the discipline of gemm_p8.hip) and the ring loop (halo_ring_loop: the weight-ring / barrier / in-wave
// fragment-prefetch structure of gemm_ring64.hip, kept as an A/B switch).  The epilogue is that of gemm_ring64.hip.
// Same-session A/B of the two loops on the headline iteration (profiles/r07_halo_loop_ab.txt: kernel trace, SQ counters, alternated bench runs):
// conv_halo_kernel family 1.17 -> 1.03 ms, MFMA busy 0.27 -> 0.32, iterations +1.8 %.  Limiter of the 8-phase loop: see the header of halo_p8_loop.
#include "epilogue.h"

namespace dpb {

typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void gbl_void_t;

__device__ inline bf16x8 halo_lds_read(unsigned addr) {
  bf16x8 v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr));
  return v;
}
__device__ inline void halo_wait_frags4(bf16x8 (&a)[2], bf16x8 (&b)[2]) {
  asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(a[0]), "+v"(a[1]), "+v"(b[0]), "+v"(b[1]));
}
__device__ inline void halo_wait_frags0(bf16x8 (&a)[2], bf16x8 (&b)[2]) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0]), "+v"(a[1]), "+v"(b[0]), "+v"(b[1]));
}
__device__ inline void halo_wait_vm(int n) {       // n in {0, 2, 4, 7, 9, 11, 13}: DMA instructions allowed to stay in flight
  if (n >= 13) asm volatile("s_waitcnt vmcnt(13)" ::: "memory");
  else if (n == 11) asm volatile("s_waitcnt vmcnt(11)" ::: "memory");
  else if (n == 9) asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
  else if (n == 7) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
  else if (n == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else if (n == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

constexpr int HALO_BM = 256, HALO_BN = 128, HALO_NH = 7;               // NH: halo DMA instructions per wave (8 x 7 x 64 >= 396 pixels x 8 chunks)
constexpr int HALO_MAXPIX = 400;
constexpr int HALO_BYTES = ((HALO_MAXPIX * 8 + 63) / 64) * 1024;        // whole wave instructions: 51,200 B
constexpr int HALO_BSTAGE = HALO_BN * 128, HALO_S = 3;
constexpr int HALO_SMEM = 2 * HALO_BYTES + HALO_S * HALO_BSTAGE + 1024;  // the larger LDS map of the two loops (ring: 3 x 16 KiB stages + sink)

// The ring loop (round 2; dpb_debug_set("halo_loop", 0) / DPB_HALO_LOOP=0): all 8 waves in lockstep, one vmcnt wait + barrier per (chunk, tap)
template <int GATHER, int FL>
__device__ __forceinline__ void halo_ring_loop(const GemmArgs& p, char* smem) {
  constexpr int BM = HALO_BM, BN = HALO_BN, WAVES = 8, NH = HALO_NH, S = HALO_S, KK = 4;
  constexpr int NIB = BN / (8 * WAVES);                                  // 2 weight DMA instructions per wave and stage
  constexpr int WN = BN / 2, SLD = WN + 4;
  constexpr int B0 = 2 * HALO_BYTES, DUMMY = B0 + S * HALO_BSTAGE;       // LDS map: halo 0 | halo 1 | weight ring | 1 KiB sink for unused DMA slots
  constexpr int SMEM_BYTES = DUMMY + 1024;
  static_assert(SMEM_BYTES >= WAVES * 32 * SLD * 4 && SMEM_BYTES <= HALO_SMEM, "LDS budget");
  const unsigned lds0 = (unsigned)(uintptr_t)(lds_void_t*)smem;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tilesN = (p.N + BN - 1) / BN, tilesM = (p.M + BM - 1) / BM;
  int lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  {
    const int nwg = gridDim.x * gridDim.y * gridDim.z, q = nwg >> 3, r = nwg & 7, xcd = lin & 7, idx = lin >> 3;
    lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  int tm, tn;
  if (p.order == 0) { tn = lin % tilesN; lin /= tilesN; tm = lin % tilesM; lin /= tilesM; }
  else { tm = lin % tilesM; lin /= tilesM; tn = lin % tilesN; lin /= tilesN; }
  const int ksplit = lin;                                                 // Z1 = Z2 = 1 (checked on the host)
  const int m0 = tm * BM, n0 = tn * BN;
  const bf16* A = (const bf16*)p.A;
  const bf16* B = (const bf16*)p.B;
  bf16* C = (bf16*)p.C;
  const bf16* R = (const bf16*)p.R;
  const bf16* zero = (const bf16*)p.zeros;

  // geometry: the tile = image rows y0 .. y0+RT-1 of one sample (H*W a multiple of 256), or SPT whole samples (H*W < 256,
  // e.g. the four 8x8 images of a 256-pixel tile), each with its own zero-padded halo
  const int W = p.W, H = p.H, Cin = p.Cin, lda = p.lda, HWp = W + 2;
  const int hw = H * W, SPT = hw >= BM ? 1 : BM / hw, RT = hw >= BM ? BM / W : H;
  const int smp = m0 / hw, y0 = hw >= BM ? (m0 - smp * hw) / W : 0, nsmp = p.M / hw;
  const int hpix = (RT + 2) * HWp, npix = SPT * hpix, tpix = RT * W;      // halo pixels per sample, per tile; output pixels per sample
  // K range in chunks of 64 input channels
  const int nch_all = Cin / 64;
  int c_begin = 0, nch = nch_all;
  if (p.splitk > 1) {
    const int per = (nch_all + p.splitk - 1) / p.splitk;
    c_begin = ksplit * per;
    nch = max(0, min(nch_all, c_begin + per) - c_begin);
  }
  const int ns = nch * 9;                                                 // stages: (chunk, tap)

  // ---- halo DMA slots: wave instruction i covers LDS chunks (wave*NH + i)*64 + lane = pixel slot>>3, physical chunk slot&7
  const bf16* h_src[NH];                                                  // source pixel's channel vector + logical chunk offset (nullptr = zero page)
  int h_dst[NH];                                                          // byte offset inside a halo buffer, or -1: sink
#pragma unroll
  for (int i = 0; i < NH; ++i) {
    const int inst = wave * NH + i, slot = inst * 64 + lane, pix = slot >> 3, phys = slot & 7;
    h_dst[i] = inst * 1024 < HALO_BYTES ? inst * 1024 : -1;
    h_src[i] = nullptr;
    if (pix < npix) {
      const int sl = pix / hpix, rp = pix - sl * hpix, hy = rp / HWp, hx = rp - hy * HWp, iy = y0 - 1 + hy, ix = hx - 1;
      if (smp + sl < nsmp && iy >= 0 && iy < H && ix >= 0 && ix < W)
        h_src[i] = A + ((long)((smp + sl) * H + iy) * W + ix) * lda + ((phys ^ ((pix >> 1) & 7)) << 3);
    }
  }
  const bf16* b_src[NIB];
#pragma unroll
  for (int i = 0; i < NIB; ++i) {
    const int pos = (wave * NIB + i) * 64 + lane, row = pos >> 3, phys = pos & 7, n = n0 + row;
    b_src[i] = n < p.N ? B + (long)n * p.ldb + ((phys ^ ((row >> 1) & 7)) << 3) : nullptr;
  }
  auto issue_halo = [&](int c) {                                          // chunk c (absolute) -> halo buffer c & 1
    char* hb = smem + (c & 1) * HALO_BYTES;
#pragma unroll
    for (int i = 0; i < NH; ++i) {
      const bf16* src = h_src[i] ? h_src[i] + c * 64 : zero;
      char* dst = h_dst[i] >= 0 ? hb + h_dst[i] : smem + DUMMY;
      __builtin_amdgcn_global_load_lds((gbl_void_t*)src, (lds_void_t*)dst, 16, 0, 0);
    }
  };
  auto issue_b = [&](int s) {                                             // stage s = (chunk c_begin + s/9, tap s%9) -> ring slot s % S
    const int c = c_begin + s / 9, tap = s - (s / 9) * 9;
    char* st = smem + B0 + (s % S) * HALO_BSTAGE;
    const int koff = tap * Cin + c * 64;
#pragma unroll
    for (int i = 0; i < NIB; ++i) {
      const bf16* src = b_src[i] ? b_src[i] + koff : zero;
      __builtin_amdgcn_global_load_lds((gbl_void_t*)src, (lds_void_t*)(st + (wave * NIB + i) * 1024), 16, 0, 0);
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int wy = wave >> 1, wx = wave & 1, l31 = lane & 31, lhi = lane >> 5;
  int pixm[2];                                                            // halo pixel of the CENTRE tap for this lane's two A-fragment rows
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = wy * 64 + i * 32 + l31, sl = m / tpix, r = m - sl * tpix, oy = r / W, ox = r - oy * W;
    pixm[i] = sl * hpix + (oy + 1) * HWp + ox + 1;
  }
  unsigned fb0[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int row = wx * WN + j * 32 + l31;
    fb0[j] = B0 + row * 128 + ((lhi ^ ((row >> 1) & 7)) << 4);
  }
  bf16x8 fa[2][2], fb[2][2];
  unsigned abase[2], asw[2];                                              // per stage: byte address of the tap's pixel, its swizzle
  auto set_stage = [&](int s) {
    const int c = c_begin + s / 9, tap = s - (s / 9) * 9, ky = (tap * 11) >> 5, kx = tap - ky * 3;
    const int toff = GATHER == GATHER_CONV ? (ky - 1) * HWp + (kx - 1) : (1 - ky) * HWp + (1 - kx);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int pix = pixm[i] + toff;
      abase[i] = lds0 + (c & 1) * HALO_BYTES + pix * 128;
      asw[i] = (pix >> 1) & 7;
    }
  };
  auto read_frags = [&](int s, int kk, int buf) {
    const unsigned sbB = lds0 + (s % S) * HALO_BSTAGE;
#pragma unroll
    for (int i = 0; i < 2; ++i) fa[buf][i] = halo_lds_read(abase[i] + ((((kk << 1) | lhi) ^ asw[i]) << 4));
#pragma unroll
    for (int j = 0; j < 2; ++j) fb[buf][j] = halo_lds_read(sbB + (fb0[j] ^ (kk << 5)));
  };

  if (ns > 0) {
    // prologue: halo(c_begin), B(0), B(1), then what the boundary before stage 0 issues: halo(c_begin + 1), B(2)
    issue_halo(c_begin);
    issue_b(0);
    if (ns > 1) issue_b(1);
    if (nch > 1) issue_halo(c_begin + 1);
    if (ns > 2) issue_b(2);
    halo_wait_vm((ns > 1 ? 2 : 0) + (nch > 1 ? NH : 0) + (ns > 2 ? 2 : 0));      // everything up to B(0) has landed
    __builtin_amdgcn_s_barrier();
    set_stage(0);
    read_frags(0, 0, 0);
    for (int s = 0; s < ns; ++s) {
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        const int cur = kk & 1, nxt = cur ^ 1;
        if (kk + 1 < KK) {
          read_frags(s, kk + 1, nxt);
          halo_wait_frags4(fa[cur], fb[cur]);
        } else {
          halo_wait_frags0(fa[cur], fb[cur]);                            // every LDS read of stage s by this wave is done
          if (s + 1 < ns) {
            const int tap_s = s - (s / 9) * 9, ch_s = s / 9;
            // B(s+1) landed: later in the queue are B(s+2) and, if stage s opened a chunk, the halo issued before it
            halo_wait_vm((s + 2 < ns ? 2 : 0) + ((tap_s == 0 && ch_s + 1 < nch) ? NH : 0));
            __builtin_amdgcn_s_barrier();                                 // stage s+1 (and its halo) visible to all; stage s consumed by all
            const int tap_n = tap_s == 8 ? 0 : tap_s + 1, ch_n = tap_s == 8 ? ch_s + 1 : ch_s;
            if (tap_n == 0 && ch_n + 1 < nch) issue_halo(c_begin + ch_n + 1);   // buffer of chunk ch_n - 1: all its stages are consumed
            if (s + 3 < ns) issue_b(s + 3);
            set_stage(s + 1);
            read_frags(s + 1, 0, nxt);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = H16<FL>::mfma(fa[cur][i], fb[cur][j], acc[i][j]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();

  // ---- epilogue through LDS: the staging layout and the slab writer of the ring kernels (epilogue.h)
  float* stage = reinterpret_cast<float*>(smem) + wave * 32 * SLD;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) stage[((r & 3) + 8 * (r >> 2) + 4 * lhi) * SLD + j * 32 + l31] = acc[i][j][r];
    __syncthreads();
    epilogue_slab<FL, WN, SLD, EPI_PLAIN>(p, C, R, reinterpret_cast<const float*>(smem), wave, lane, m0 + wy * 64 + i * 32, n0, (long)ksplit);
    __syncthreads();
  }
}

// ---- the 8-phase loop (default): the discipline of gemm_p8.hip on the halo tile
template <int OFF>
__device__ __forceinline__ bf16x8 halo_read_at(unsigned addr) {
  bf16x8 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}
// s_waitcnt lgkmcnt(0) the compiler must keep between the fragment reads and the MFMAs that consume them (the fragments are threaded through it)
__device__ __forceinline__ void halo_wait12(bf16x8 (&a)[2][4], bf16x8 (&b)[4]) {
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(a[0][0]), "+v"(a[0][1]), "+v"(a[0][2]), "+v"(a[0][3]), "+v"(a[1][0]), "+v"(a[1][1]), "+v"(a[1][2]), "+v"(a[1][3]), "+v"(b[0]), "+v"(b[1]),
                 "+v"(b[2]), "+v"(b[3]));
}
__device__ __forceinline__ void halo_wait4(bf16x8 (&b)[4]) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]));
}

constexpr int HP8_PH = 18, HP8_LOOK = 4, HP8_SLOTS = 6, HP8_HALF = 64 * 128;   // phases per chunk, DMA lookahead (phases), weight-ring slots, half tile bytes
// The counted wait of phase j of a chunk (see the header of halo_p8_loop): the half tile read in phase j+1 was the last DMA of phase j+1-LOOK; younger are
// the LOOK-1 half tiles of the phases after it and the halo pieces issued in those phases and in phase j (piece i in phase i, ahead of the half tile).
constexpr int hp8_vm(int j) {
  int n = HP8_LOOK - 1;
  for (int t = j - (HP8_LOOK - 2); t <= j; ++t) n += (t >= 0 && t < HALO_NH);
  return n;
}

// Wave (wy, wx) = (wave >> 1, wave & 1) owns the 64 x 64 output tile at rows wy * 64, columns wx * 64 of the 256 x 128 block tile, as in the ring loop;
// group g = wave >> 2 (waves w and w + 4 share a SIMD: one of each group on every SIMD).  Stage (chunk, tap) is cut into two phases, one per 32-column
// B half (LDS half tile h holds tile columns (r >> 5) * 64 + h * 32 + (r & 31), r = 0..63: every wave reads 32 rows of each half):
//   phase 2t:   read A(tap) (8) + B0 (4) | halo piece 2t of chunk c+1 (t < 4) | half tile of phase 2t+4 | vmcnt | barrier | lgkmcnt(0) | 8 MFMA a x b0 | barrier
//   phase 2t+1: read B1 (4)              | halo piece 2t+1 (2t+1 < 7)         | half tile of phase 2t+5 | vmcnt | barrier | lgkmcnt(0) | 8 MFMA a x b1 | barrier
// One DMA instruction per wave moves a half tile (8 waves x 1 KiB); the chunk's 50 KiB halo is 7 instructions per wave, issued one per phase in phases
// 0-6 of the chunk before it.  18 phases per chunk, the chunk body unrolled: the ring slot of every half tile (phase % 6) and the wait of every phase are
// static.  The two groups run ONE BARRIER APART (group 0 ahead), so on each SIMD one wave issues MFMAs while its partner reads fragments / issues DMA.
// Ordering rules (as in gemm_p8.hip, barriers counted per phase: a wave's load segment ends at the phase's first barrier, its matrix segment at the second):
//   RAW  a buffer is read one phase AFTER the phase whose vmcnt covers it in every wave: the half tile of phase q is issued in phase q-4 and covered by the
//        wait of phase q-1 (vmcnt = 3 half tiles + the halo pieces of phases q-3..q-1 behind it: hp8_vm); the halo of chunk c+1 (phases 0-6 of chunk c) is
//        covered by the wait of phase 17 of chunk c at the latest and first read in phase 0 of chunk c+1.
//   WAR  a buffer is restaged two phases after its last read, whose lgkmcnt(0) precedes the reading phase's SECOND barrier: ring slot q % 6 is read in
//        phase q and restaged in phase q+2 (half tile of phase q+6); halo buffer (c+1) & 1 was last read in phase 16 of chunk c-1 (tap 8) and is restaged
//        from phase 0 of chunk c.
// Half tiles and halo pieces "after the end" of the block's chunk range (and N-tail columns) read the zero page, so the DMA count per phase is static.
// K order per output element: chunk, tap, K16 substep -- that of the ring loop, so the two loops agree bit for bit (and split-K partitions chunks alike).
// Wave tile: 64 x 64 gives 1 KiB of LDS reads per 32x32x16 MFMA (2 + 2 fragments per 4 MFMAs); the 128 x 32 alternative on a 256 x 128 tile needs 1.25 KiB,
// and a 256 x 256 block tile (0.75 KiB, p8's 128 x 64 wave tile) leaves no LDS for a double-buffered halo: 100 KiB of halos + 64 KiB of weight parities.
// Registers: 64 accumulators + 32 (A) + 2 x 16 (B) fragment VGPRs.  LDS: 2 x 50 KiB halos + 6 x 8 KiB weight slots + 1 KiB sink = 149 KiB.
// Measured limiter (profiles/r07_halo_loop_ab.txt): against the ring loop wave cycles fall 17 % but the issue wait rises from 0.33 to 0.44 of them.
// The matrix segment of a phase waits (lgkmcnt(0)) for the fragments read in the same phase's load segment; the even phase reads 12 of them, more
// than the partner group's 8 MFMAs cover, and the stall is paid at a block barrier, 36 of them per chunk.  The DMA stream is not the limiter
// (~22 KiB per stage: ~550 cycles at 40 B/clk/CU against 1024 MFMA cycles per SIMD).  Reading fragments one phase ahead is the next step.
template <int GATHER, int FL>
__device__ __forceinline__ void halo_p8_loop(const GemmArgs& p, char* smem) {
  constexpr int BM = HALO_BM, BN = HALO_BN, NH = HALO_NH, PH = HP8_PH, LOOK = HP8_LOOK, NSLOT = HP8_SLOTS, HALF = HP8_HALF;
  constexpr int WN = BN / 2, SLD = WN + 4;
  constexpr int B0 = 2 * HALO_BYTES, SINK = B0 + NSLOT * HALF;      // LDS map: halo 0 | halo 1 | 6 half-tile slots | 1 KiB sink for unused DMA slots
  static_assert(SINK + 1024 <= HALO_SMEM && 8 * 32 * SLD * 4 <= HALO_SMEM, "LDS budget");
  static_assert(HALF == 8 * 1024 && BN == 128, "a half tile = 64 columns x 64 channels = one 1 KiB DMA instruction per wave");
  static_assert(NSLOT >= LOOK + 2 && PH % NSLOT == 0 && PH % 2 == 0, "WAR: a slot is restaged >= 2 phases after its read; static slots per chunk");
  static_assert(NH <= PH - LOOK + 1 && NH <= 7, "the halo of chunk c+1 is covered by the waits of chunk c");
  static_assert(hp8_vm(0) == 4 && hp8_vm(2) == 6 && hp8_vm(7) == 5 && hp8_vm(9) == 3, "the counted waits of the header");
  static_assert((NSLOT - 1) * HALF < 65536, "slot offsets are ds_read immediates");
  const unsigned lds0 = (unsigned)(uintptr_t)(lds_void_t*)smem;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tilesN = (p.N + BN - 1) / BN, tilesM = (p.M + BM - 1) / BM;
  int lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  {
    const int nwg = gridDim.x * gridDim.y * gridDim.z, q = nwg >> 3, r = nwg & 7, xcd = lin & 7, idx = lin >> 3;
    lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  int tm, tn;
  if (p.order == 0) { tn = lin % tilesN; lin /= tilesN; tm = lin % tilesM; lin /= tilesM; }
  else { tm = lin % tilesM; lin /= tilesM; tn = lin % tilesN; lin /= tilesN; }
  const int ksplit = lin;
  const int m0 = tm * BM, n0 = tn * BN;
  const bf16* A = (const bf16*)p.A;
  const bf16* B = (const bf16*)p.B;
  bf16* C = (bf16*)p.C;
  const bf16* R = (const bf16*)p.R;
  const bf16* zero = (const bf16*)p.zeros;

  // geometry and chunk range: those of the ring loop
  const int W = p.W, H = p.H, Cin = p.Cin, lda = p.lda, HWp = W + 2;
  const int hw = H * W, SPT = hw >= BM ? 1 : BM / hw, RT = hw >= BM ? BM / W : H;
  const int smp = m0 / hw, y0 = hw >= BM ? (m0 - smp * hw) / W : 0, nsmp = p.M / hw;
  const int hpix = (RT + 2) * HWp, npix = SPT * hpix, tpix = RT * W;
  const int nch_all = Cin / 64;
  int c_begin = 0, nch = nch_all;
  if (p.splitk > 1) {
    const int per = (nch_all + p.splitk - 1) / p.splitk;
    c_begin = ksplit * per;
    nch = max(0, min(nch_all, c_begin + per) - c_begin);
  }

  const bf16* h_src[NH];                                                  // halo piece i: as in the ring loop (nullptr = zero page)
  int h_dst[NH];                                                          // byte offset inside a halo buffer, or -1: sink
#pragma unroll
  for (int i = 0; i < NH; ++i) {
    const int inst = wave * NH + i, slot = inst * 64 + lane, pix = slot >> 3, phys = slot & 7;
    h_dst[i] = inst * 1024 < HALO_BYTES ? inst * 1024 : -1;
    h_src[i] = nullptr;
    if (pix < npix) {
      const int sl = pix / hpix, rp = pix - sl * hpix, hy = rp / HWp, hx = rp - hy * HWp, iy = y0 - 1 + hy, ix = hx - 1;
      if (smp + sl < nsmp && iy >= 0 && iy < H && ix >= 0 && ix < W)
        h_src[i] = A + ((long)((smp + sl) * H + iy) * W + ix) * lda + ((phys ^ ((pix >> 1) & 7)) << 3);
    }
  }
  const bf16* b_src[2];                                                   // half h: lane's 16-byte piece, LDS row r = (wave * 64 + lane) >> 3
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int pos = wave * 64 + lane, r = pos >> 3, phys = pos & 7, n = n0 + (r >> 5) * 64 + h * 32 + (r & 31);
    b_src[h] = n < p.N ? B + (long)n * p.ldb + ((phys ^ ((r >> 1) & 7)) << 3) : nullptr;
  }
  auto issue_halo = [&](auto ic, int c) {                                 // piece i of chunk c (relative) -> halo buffer c & 1
    constexpr int i = decltype(ic)::value;
    const bf16* src = (h_src[i] && c < nch) ? h_src[i] + (c_begin + c) * 64 : zero;
    char* dst = h_dst[i] >= 0 ? smem + (c & 1) * HALO_BYTES + h_dst[i] : smem + SINK;
    __builtin_amdgcn_global_load_lds((gbl_void_t*)src, (lds_void_t*)dst, 16, 0, 0);
  };
  auto issue_b = [&](auto jc, int c) {                                    // half tile of phase j of chunk c (relative) -> ring slot j % NSLOT
    constexpr int j = decltype(jc)::value, h = j & 1, tap = j >> 1, slot = j % NSLOT;
    const bf16* src = (b_src[h] && c < nch) ? b_src[h] + tap * Cin + (c_begin + c) * 64 : zero;
    __builtin_amdgcn_global_load_lds((gbl_void_t*)src, (lds_void_t*)(smem + B0 + slot * HALF + wave * 1024), 16, 0, 0);
  };

  f32x16 acc[2][2];                                                       // [32-row fragment][B half]
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int wy = wave >> 1, wx = wave & 1, l31 = lane & 31, lhi = lane >> 5;
  int pixm[2];                                                            // halo pixel of the CENTRE tap for this lane's two A-fragment rows
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = wy * 64 + i * 32 + l31, sl = m / tpix, r = m - sl * tpix, oy = r / W, ox = r - oy * W;
    pixm[i] = sl * hpix + (oy + 1) * HWp + ox + 1;
  }
  unsigned adB[4];                                                        // B fragment: row wx * 32 + l31 of a half, K16 substep kk; slot = immediate
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const int r = wx * 32 + l31;
    adB[kk] = lds0 + B0 + r * 128 + ((((kk << 1) | lhi) ^ ((r >> 1) & 7)) << 4);
  }
  bf16x8 fa[2][4], fb0[4], fb1[4];
  auto read_a = [&](auto tc, int c) {
    constexpr int tap = decltype(tc)::value, ky = tap / 3, kx = tap % 3;
    const int toff = GATHER == GATHER_CONV ? (ky - 1) * HWp + (kx - 1) : (1 - ky) * HWp + (1 - kx);
    const unsigned hb = lds0 + (c & 1) * HALO_BYTES;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int pc = pixm[i];
      asm volatile("" : "+v"(pc));        // opaque per phase: keeps the compiler from hoisting the 9 taps' 72 fragment addresses out of the chunk loop
      const int pix = pc + toff, sw = (pix >> 1) & 7;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) fa[i][kk] = halo_lds_read(hb + pix * 128 + ((((kk << 1) | lhi) ^ sw) << 4));
    }
  };
  auto read_b = [&](auto sc, bf16x8 (&fb)[4]) {
    constexpr int o = decltype(sc)::value * HALF;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) fb[kk] = halo_read_at<o>(adB[kk]);
  };
  auto mma = [&](auto hc, bf16x8 (&fb)[4]) {
    constexpr int h = decltype(hc)::value;
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      acc[0][h] = H16<FL>::mfma(fa[0][kk], fb[kk], acc[0][h]);
      acc[1][h] = H16<FL>::mfma(fa[1][kk], fb[kk], acc[1][h]);
    }
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
  };
  auto bar = [&]() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;

  auto phase = [&](auto jc, int c) {                                      // phase j of chunk c (relative)
    constexpr int j = decltype(jc)::value, tap = j >> 1, h = j & 1, jn = j + LOOK;
    using SLOT = std::integral_constant<int, j % NSLOT>;
    if constexpr (h == 0) {
      read_a(std::integral_constant<int, tap>{}, c);
      read_b(SLOT{}, fb0);
    } else {
      read_b(SLOT{}, fb1);
    }
    if constexpr (j < NH) issue_halo(jc, c + 1);
    if constexpr (jn < PH) issue_b(std::integral_constant<int, jn>{}, c);
    else issue_b(std::integral_constant<int, jn - PH>{}, c + 1);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(hp8_vm(j)) : "memory");      // the half tile of phase j+1 (and, by phase 17, the next chunk's halo) landed
    bar();
    if constexpr (h == 0) {
      halo_wait12(fa, fb0);
      mma(I0{}, fb0);
    } else {
      halo_wait4(fb1);
      mma(I1{}, fb1);
    }
    bar();
  };

  if (nch > 0) {
    static_for<0, NH>([&](auto ic) { issue_halo(ic, 0); });              // prologue: halo of chunk 0, half tiles of phases 0-3
    static_for<0, LOOK>([&](auto jc) { issue_b(jc, 0); });
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LOOK - 1) : "memory");      // halo 0 and the half tile of phase 0 landed
    bar();
    if (wave >= 4) bar();                                                 // group 1 runs one barrier behind group 0 from here on
    for (int c = 0; c < nch; ++c) static_for<0, PH>([&](auto jc) { phase(jc, c); });
    if (wave < 4) bar();
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();

  // ---- epilogue: that of the ring loop
  float* stage = reinterpret_cast<float*>(smem) + wave * 32 * SLD;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) stage[((r & 3) + 8 * (r >> 2) + 4 * lhi) * SLD + j * 32 + l31] = acc[i][j][r];
    __syncthreads();
    epilogue_slab<FL, WN, SLD, EPI_PLAIN>(p, C, R, reinterpret_cast<const float*>(smem), wave, lane, m0 + wy * 64 + i * 32, n0, (long)ksplit);
    __syncthreads();
  }
}

// LOOP: 1 the 8-phase loop (default), 0 the ring loop (dpb_debug_set("halo_loop", 0) or DPB_HALO_LOOP=0: same results bit for bit, an A/B switch)
template <int GATHER, int FL, int LOOP>   // FL: 16-bit flavour (H16<FL>): 0 bf16, 1 f16
__global__ __launch_bounds__(512) void conv_halo_kernel(GemmArgs p) {
  __shared__ __attribute__((aligned(1024))) char smem[HALO_SMEM];
  if constexpr (LOOP) halo_p8_loop<GATHER, FL>(p, smem);
  else halo_ring_loop<GATHER, FL>(p, smem);
}

// 3x3, stride 1, pad 1, forward gather or its adjoint; whole image rows (or whole small images) per tile; 64-channel chunks
int conv_halo_supported(const GemmArgs& a) {
  if (a.gather != GATHER_CONV && a.gather != GATHER_CONVT) return 0;
  if (a.KS != 3 || a.stride != 1 || a.pad != 1 || a.Z1 * a.Z2 != 1 || a.A2) return 0;
  if (a.H != a.Ho || a.W != a.Wo || a.Cin % 64 || a.K != 9 * a.Cin) return 0;
  const int hw = a.H * a.W;
  if (a.M % hw) return 0;
  if (hw >= HALO_BM) {                              // whole image rows of one sample per tile
    if (HALO_BM % a.W || hw % HALO_BM) return 0;
    if ((HALO_BM / a.W + 2) * (a.W + 2) > HALO_MAXPIX) return 0;
  } else {                                          // whole samples per tile (8x8: four)
    if (HALO_BM % hw || a.W < 8) return 0;
    if ((HALO_BM / hw) * (a.H + 2) * (a.W + 2) > HALO_MAXPIX) return 0;
  }
  if (a.lda % 8 || a.ldb % 8 || !a.zeros) return 0;
  return 1;
}

static int g_halo_loop = 1;
void conv_halo_debug_loop(int on) { g_halo_loop = on; }

template <int GATHER, int FL>
static void launch_halo_g(const GemmArgs& a, dim3 grid, hipStream_t st) {
  static const int loop_env = getenv("DPB_HALO_LOOP") ? atoi(getenv("DPB_HALO_LOOP")) : 1;   // A/B switch (0: the ring loop)
  if (loop_env && g_halo_loop) DPB_LAUNCH((conv_halo_kernel<GATHER, FL, 1>), grid, dim3(512), 0, st, a);
  else DPB_LAUNCH((conv_halo_kernel<GATHER, FL, 0>), grid, dim3(512), 0, st, a);
}

int launch_conv_halo(const GemmArgs& a, hipStream_t st) {
  const int sk = a.splitk > 1 ? a.splitk : 1;
  dim3 grid(((a.M + HALO_BM - 1) / HALO_BM) * ((a.N + HALO_BN - 1) / HALO_BN), 1, sk);
  if (a.gather == GATHER_CONV) {
    if (a.fl) launch_halo_g<GATHER_CONV, 1>(a, grid, st);
    else launch_halo_g<GATHER_CONV, 0>(a, grid, st);
  } else {
    if (a.fl) launch_halo_g<GATHER_CONVT, 1>(a, grid, st);
    else launch_halo_g<GATHER_CONVT, 0>(a, grid, st);
  }
  DPB_CHECK(hipGetLastError());
  return 0;
}

}  // namespace dpb
