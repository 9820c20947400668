// Host-side launch interface of the gfx950 kernels (internal; the public C-ABI is include/dpb.h).
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <type_traits>
#include <utility>

#include "common.h"

namespace dpb {

// ---------------------------------------------------------------- GEMM / implicit-GEMM convolution
// C[z][m][n] = alpha * sum_k A[z][m][k] * B[z][n][k]  (+bias[n]) (+rowbias[sample(m)][n]) (+R[z][m][n]) (+C if accumulate)
// A: plain rows (lda) or gathered NHWC pixels (conv).  B is always [N][K], K contiguous.
enum { GATHER_NONE = 0, GATHER_CONV = 1, GATHER_CONVT = 2, GATHER_UPCONV = 3 };
enum { EPI_PLAIN = 0, EPI_GEGLU_TAN = 1, EPI_GEGLU_ADJ = 2, EPI_LN_TAN = 3, EPI_LN_ADJ = 4, EPI_GEGLU_FWD = 5, EPI_XATT = 6 };   // fused epilogues of the ring GEMMs (epilogue.h)
struct GemmArgs {
  const void* A = nullptr; const void* B = nullptr; void* C = nullptr; const void* R = nullptr;
  const float* bias = nullptr;
  const void* rowbias = nullptr;      // [samples][ldrb] in T, the first N columns of a row are this product's; sample(m) = (m / rows_per_sample) / rowbias_div
  int rows_per_sample = 1, rowbias_div = 1;
  int ldrb = 0;                       // row pitch of rowbias in elements (a column window of a wider buffer: not N); multiplies sample(m), so one shared row needs none
  int M = 0, N = 0, K = 0;
  int lda = 0, ldb = 0, ldc = 0, ldr = 0;
  // two-level batch z = z1 * Z2 + z2 ; per-operand offset = (z1 / div) * s1 + z2 * s2  (elements)
  int Z1 = 1, Z2 = 1;
  long sA1 = 0, sA2 = 0, sB1 = 0, sB2 = 0, sC1 = 0, sC2 = 0, sR1 = 0, sR2 = 0;
  int divA = 1, divB = 1;
  float alpha = 1.f;
  int accumulate = 0;
  // gather description (A is [samples][H*W][Cin] NHWC, output pixels Ho x Wo, KS x KS taps)
  int gather = GATHER_NONE;
  int H = 0, W = 0, Cin = 0, Ho = 0, Wo = 0, KS = 1, stride = 1, pad = 0;
  // optional second operand pair appended to the K loop (plain rows only)
  const void* A2 = nullptr; const void* B2 = nullptr;
  int K2 = 0, lda2 = 0, ldb2 = 0, divA2 = 1, divB2 = 1;
  long sA21 = 0, sA22 = 0, sB21 = 0, sB22 = 0;
  // split-K scratch (fp32 slabs); splitk / vec_ok are filled in by launch_gemm
  float* slab = nullptr; size_t slab_bytes = 0;
  const void* zeros = nullptr;        // >= 16 zero bytes in device memory (DMA kernel reads it for padding / out-of-range rows)
  int splitk = 1, vec_ok = 0;
  // fused GEGLU epilogues (ring kernels with 128-column tiles, no split-K): primal FF-in output [prows][2F], columns interleaved in
  // blocks of 64 (a | g); tangent row m belongs to primal sample (m / rows_per_sample) / epi_kps
  int epi = EPI_PLAIN, epi_kps = 1;
  const void* hprim = nullptr;
  // fused LayerNorm epilogues (row-complete 128 x 320 tile, gemm_ring64.hip): EPI_LN_TAN writes h = acc (+R) to C AND its LayerNorm tangent to C2;
  // EPI_LN_ADJ adds the LayerNorm adjoint of the product (the cotangent of the LayerNorm OUTPUT) to C.  ln_x: primal LayerNorm input [prows][N]
  // (row m belongs to primal row ((m / rows_per_sample) / epi_kps) * rows_per_sample + m % rows_per_sample), ln_gamma fp32 [N]
  const void* ln_x = nullptr; const float* ln_gamma = nullptr; float ln_eps = 1e-5f; void* C2 = nullptr;
  // folded text-attention epilogue (EPI_XATT, 128-column tiles of gemm_ring64.hip, no split-K): one 128-column tile is one head's scores against the
  // folded operand (xatt_lk live columns, the rest of the window padding); with the primal probabilities xatt_p fp32 [prows][xatt_h][80] (row
  // indexing as hprim) the tile leaves as w = P o (acc - sum_j P_j acc_j), columns j < 80 stored compactly at C[m][80 h + j] (ldc = 80 xatt_h)
  const float* xatt_p = nullptr; int xatt_h = 0, xatt_lk = 0;
  int fl = 0;                         // 16-bit flavour of the specialised kernels: 0 bf16, 1 f16 (filled in by launch_gemm)
  int order = 0;                      // block processing order per XCD: 0 A-major, 1 B-major (weight-heavy); filled in by launch_gemm
};
// ---- the tile table: ONE row per tile the library can launch.  Everything the host code knows about a tile -- its geometry, its codes, which
// launcher and which kernel variants it has, how the profile labels it -- is read from its row; a new tile is a new row (and its kernel).
enum GemmFamily { FAM_REG = 0, FAM_RING32, FAM_RING64, FAM_P8, FAM_WRES, FAM_HALO };   // gemm.hip | gemm_dma.hip | gemm_ring64.hip | gemm_p8.hip | gemm_wres.hip | gemm_halo.hip
enum : unsigned {
  TILE_CONV = 1,      // takes the forward / transposed gathers (GATHER_CONV, GATHER_CONVT), plain epilogue
  TILE_UPCONV = 2,    // ... and the upsampling gather
  TILE_CIN64 = 4,     // gathers whole 64-channel K tiles only (Cin % 64 == 0)
  TILE_GEGLU = 8,     // built with the fused GEGLU epilogues (plain rows); the dispatch uses them on tiles of whole 128-column blocks only
  TILE_LN = 16,       // the row-complete tile: built with the fused LayerNorm epilogues and nothing else; N = bn, selected by the epilogue, never forced
  TILE_EPI_N256 = 32, // fused epilogues need N % 256 == 0
  TILE_NOSPLIT = 64,  // one block per CU by construction: the heuristic never splits K (a forced split count is honoured)
  TILE_NOSLAB = 128,  // no split-K path at all: one K range per block whatever is forced
  TILE_XATT = 256,    // built with the folded text-attention epilogue (EPI_XATT, plain rows)
};
enum GemmTileId { T_REG64 = 0, T_REG128, T_R32_S4, T_R32_S3, T_R32_S2, T_R32_TALL, T_R32_64, T_R32_64B, T_R64_S3, T_R64_TALL, T_R64_S4, T_R64_S2, T_R64_TALL8,
                  T_R64_TALL8_S2, T_R64_256, T_R64_LN, T_R64_HALF, T_R64_HALF_S2, T_R64_HALFN, T_P8, T_WRES, T_HALO, GEMM_TILES, T_NONE = -1 };
struct GemmTile {
  int family;
  int code;        // what gemm_plan / dpb_debug_gemm_plan report
  int forced;      // what dpb_debug_set("gemm_tile") / DPB_GEMM_OVERRIDE accept (0: not forceable)
  int bm, bn, stages, waves;
  int kind;        // profile kind of dpb_engine_profile_read (include/dpb.h)
  unsigned flags;
  int substitute;  // the row a forced code falls back to for a product this tile does not take (T_NONE: forced unconditionally)
};
constexpr unsigned TILE_ANY = TILE_CONV | TILE_UPCONV;
inline constexpr GemmTile kGemmTiles[GEMM_TILES] = {
    //  family     code forced  bm   bn   S  waves kind  flags                                                          substitute
    {FAM_REG,      64,  64,    64,  64,  0, 4,    0,    TILE_ANY,                                                      T_NONE},   // register-staged (all dtypes, dual operand pairs)
    {FAM_REG,      128, 128,   128, 128, 0, 4,    1,    TILE_ANY,                                                      T_NONE},
    {FAM_RING32,   128, 129,   128, 128, 4, 4,    2,    TILE_ANY | TILE_GEGLU,                                         T_NONE},
    {FAM_RING32,   130, 131,   128, 128, 3, 4,    2,    TILE_ANY | TILE_GEGLU,                                         T_NONE},   // 48 KiB ring -> 3 blocks/CU
    {FAM_RING32,   132, 133,   128, 128, 2, 4,    2,    TILE_ANY | TILE_GEGLU,                                         T_NONE},
    {FAM_RING32,   256, 257,   256, 128, 3, 4,    2,    TILE_ANY | TILE_GEGLU,                                         T_NONE},   // wave tile 128x64, 72 KiB ring
    {FAM_RING32,   64,  65,    64,  64,  4, 4,    3,    TILE_ANY | TILE_GEGLU,                                         T_NONE},   // (its GEGLU variants are built, never dispatched)
    {FAM_RING32,   66,  67,    64,  64,  4, 4,    3,    TILE_ANY | TILE_GEGLU,                                         T_NONE},   // an alias of 65: the same launch under its own codes
    {FAM_RING64,   512, 512,   128, 128, 3, 4,    4,    TILE_ANY | TILE_GEGLU,                                         T_NONE},   // 96 KiB ring, 1 block/CU
    {FAM_RING64,   513, 513,   256, 128, 3, 4,    4,    TILE_ANY | TILE_GEGLU,                                         T_NONE},   // 144 KiB
    {FAM_RING64,   514, 514,   128, 128, 4, 4,    4,    TILE_ANY | TILE_GEGLU,                                         T_NONE},
    {FAM_RING64,   515, 515,   128, 128, 2, 4,    4,    TILE_ANY | TILE_GEGLU | TILE_XATT,                                      T_NONE},   // 2 blocks/CU: the default ring
    {FAM_RING64,   516, 516,   256, 128, 3, 8,    4,    TILE_ANY | TILE_GEGLU,                                         T_NONE},   // 64x64 wave tiles, one shared B tile
    {FAM_RING64,   517, 517,   256, 128, 2, 8,    4,    TILE_ANY | TILE_GEGLU,                                         T_NONE},   // 96 KiB
    {FAM_RING64,   518, 518,   256, 256, 2, 8,    6,    TILE_GEGLU | TILE_EPI_N256 | TILE_NOSPLIT,                     T_R64_S2}, // 64x128 wave tiles, 128 KiB ring: half the L2->LDS bytes per flop of 128x128; plain rows only
    {FAM_RING64,   520, 0,     128, 320, 2, 4,    4,    TILE_LN | TILE_NOSLAB,                                         T_NONE},   // row-complete N = 320 tile, fused LayerNorm epilogue
    {FAM_RING64,   521, 521,   64,  128, 3, 4,    4,    TILE_CONV | TILE_XATT,                                         T_R64_S2}, // half tiles for launches of <= 256 tiles: 72 KiB ring, 2 blocks/CU (also as an implicit-GEMM convolution)
    {FAM_RING64,   522, 522,   64,  128, 2, 4,    4,    0,                                                             T_R64_S2}, // 48 KiB ring: 3 blocks/CU
    {FAM_RING64,   523, 523,   128, 64,  3, 4,    4,    0,                                                             T_R64_S2},
    {FAM_P8,       530, 530,   256, 256, 2, 8,    11,   TILE_ANY | TILE_CIN64 | TILE_GEGLU | TILE_EPI_N256 | TILE_NOSPLIT, T_R64_S2}, // 8-phase ping-pong loop, 256x256x64
    {FAM_WRES,     540, 540,   32,  320, 0, 5,    12,   TILE_NOSLAB,                                                   T_R64_S2}, // weights-resident streaming: 32-row tiles past a resident 320-column weight slice (gemm_wres_supported)
    {FAM_HALO,     600, 600,   256, 128, 0, 8,    5,    TILE_CONV | TILE_CIN64,                                        T_NONE},   // halo-tile 3x3 convolution (conv_halo_supported)
};
constexpr const GemmTile* gemm_tile_forced(int forced) {   // the lookup by code: the forced codes are the unique ones (64 / 128 name a register-staged AND a ring tile as plan codes)
  for (const GemmTile& t : kGemmTiles)
    if (forced && t.forced == forced) return &t;
  return nullptr;
}
constexpr int gemm_plan_kind(const GemmTile& t) { return t.family == FAM_REG ? (t.bm == 128) : t.family == FAM_HALO ? 3 : 2; }
// which (gather, epilogue) variants of a tile's kernel are built -- the launchers instantiate exactly these, the dispatch never plans another
constexpr bool gemm_tile_builds(const GemmTile& t, int gather, int epi) {
  if (gather == GATHER_UPCONV ? !(t.flags & TILE_UPCONV) : (gather != GATHER_NONE && !(t.flags & TILE_CONV))) return false;
  if (epi == EPI_PLAIN) return !(t.flags & TILE_LN);
  if (gather != GATHER_NONE) return false;
  if (epi == EPI_XATT) return (t.flags & TILE_XATT) != 0;
  return (t.flags & ((epi == EPI_LN_TAN || epi == EPI_LN_ADJ) ? TILE_LN : TILE_GEGLU)) != 0;
}
inline long gemm_tile_count(const GemmTile& t, const GemmArgs& a) { return (long)((a.M + t.bm - 1) / t.bm) * ((a.N + t.bn - 1) / t.bn) * a.Z1 * a.Z2; }
inline dim3 gemm_tile_grid(const GemmTile& t, const GemmArgs& a) { return dim3(((a.M + t.bm - 1) / t.bm) * ((a.N + t.bn - 1) / t.bn), a.Z1 * a.Z2, a.splitk > 1 ? a.splitk : 1); }
// The launchers of the ring families: runs launch(row, fl, epi, gather) -- four std::integral_constant tags: the index of `t` in the table and the
// (GemmArgs::fl, epi, gather) of `a` -- if `t` is a row of family FAM and that variant of its kernel is built; an error otherwise.
template <int V> using GemmTag = std::integral_constant<int, V>;
template <int... Vs, typename F>
int gemm_tag_switch(int v, F&& f) {   // f(GemmTag<V>{}) for the V of Vs... that equals v; -1 if none does
  int r = -1;
  (void)((v == Vs && ((r = f(GemmTag<Vs>{})), true)) || ...);
  return r;
}
void gemm_variant_error(const GemmTile& t, const GemmArgs& a);
template <int FAM, typename F, int... Is>
int gemm_family_launch(const GemmArgs& a, const GemmTile& t, F&& launch, std::integer_sequence<int, Is...>) {
  const int r = gemm_tag_switch<Is...>((int)(&t - kGemmTiles), [&](auto row) {
    return gemm_tag_switch<0, 1>(a.fl, [&](auto fl) {
      return gemm_tag_switch<EPI_PLAIN, EPI_GEGLU_TAN, EPI_GEGLU_ADJ, EPI_LN_TAN, EPI_LN_ADJ, EPI_GEGLU_FWD, EPI_XATT>(a.epi, [&](auto epi) {
        return gemm_tag_switch<GATHER_NONE, GATHER_CONV, GATHER_CONVT, GATHER_UPCONV>(a.gather, [&](auto gather) {
          constexpr GemmTile R = kGemmTiles[decltype(row)::value];
          if constexpr (R.family == FAM && gemm_tile_builds(R, decltype(gather)::value, decltype(epi)::value)) { launch(row, fl, epi, gather); return 0; }
          else return -1;
        });
      });
    });
  });
  if (r) gemm_variant_error(t, a);
  return r;
}
using GemmTileSeq = std::make_integer_sequence<int, GEMM_TILES>;

// The launch plan of one product: its tile row (nullptr: refused, dpb_last_error says why) and K split.  kind / tile: what dpb_debug_gemm_plan reports.
struct GemmPlan { int kind, tile, splitk; const GemmTile* row; };   // kind: gemm_plan_kind(*row), -1 error; tile: row->code
// `pending` != nullptr: if the launch is split over K and its epilogue is plain
// (one batch entry, alpha 1, no bias / row bias / accumulate, dense rows), the reduce kernel is NOT launched -- *pending receives the prepared
// arguments (pending->splitk > 1) and the caller either hands the slabs to a consumer that reduces them itself (SlabSrc, norm.hip) or calls
// launch_gemm_reduce; otherwise pending->splitk is set to 1.  `plan`: the gemm_plan of these arguments if the caller already asked for it.
int launch_gemm(int dtype, const GemmArgs& a, hipStream_t st, GemmArgs* pending = nullptr, const GemmPlan* plan = nullptr);
int launch_gemm_reduce(int dtype, const GemmArgs& pending, hipStream_t st);
GemmPlan gemm_plan(int dtype, const GemmArgs& a);   // host-only: the tile launch_gemm picks, with its K split (clamped to the slab scratch)
void gemm_debug_set(int tile, int splitk, int kch);   // tuning overrides for micro-benchmarks (0 = heuristic): forced code, split count, K chunks of the 64x64 register-staged tile
int launch_gemm_dma(const GemmArgs& a, const GemmTile& t, hipStream_t st);      // BK = 32 LDS ring, 16-bit, single operand pair (gemm_dma.hip): the FAM_RING32 rows
int launch_gemm_ring64(const GemmArgs& a, const GemmTile& t, hipStream_t st);   // BK = 64 ring (gemm_ring64.hip): the FAM_RING64 rows
bool gemm_p8_fits32(const GemmArgs& a);                                // its 32-bit element offsets reach every operand row
int launch_gemm_p8(const GemmArgs& a, int tile, hipStream_t st);      // 8-phase ping-pong loop (gemm_p8.hip): the FAM_P8 row, by its code
int conv_halo_supported(const GemmArgs& a);                        // 3x3 stride-1 convolution in halo-tile form (gemm_halo.hip)
int launch_conv_halo(const GemmArgs& a, hipStream_t st);
void conv_halo_debug_loop(int on);   // 1 (default): the 8-phase main loop of the halo convolution; 0: the ring loop, bitwise A/B
int gemm_epi_supported(int dtype, const GemmArgs& a);   // can this launch take GemmArgs::epi != EPI_PLAIN?
void gemm_debug_dma_auto(int on);
void gn_debug_deterministic(int on);
int gn_deterministic();
bool gemm_wres_supported(int dtype, const GemmArgs& a);                // weights-resident streaming kernel (gemm_wres.hip): K = 320, N % 320 == 0, plain epilogue
int launch_gemm_wres(const GemmArgs& a, hipStream_t st);
void gemm_debug_wres(int on);   // 1 (default): the dispatch may pick the weights-resident kernel; 0: round-5 dispatch, bitwise A/B
void gemm_debug_p8(int on);     // 1 (default): the dispatch may pick the 8-phase tile; 0: round-4 dispatch (rings / halo kernel), bitwise A/B
void gemm_debug_order(int o);   // -1 heuristic, 0 A-major, 1 B-major

// ---------------------------------------------------------------- normalisation
enum { MODE_PRIMAL = 0, MODE_TANGENT = 1, MODE_ADJOINT = 2 };
// A deferred split-K reduction handed to the normalisation kernel that consumes the product: its tangent / cotangent input d[row][c..] is
// sum_s slab[s][row][c..] (+ R[row][c..]), added in slab order and rounded to the engine dtype exactly as splitk_reduce_kernel would have
// stored it (bitwise the same values), optionally written to `store` when another op reads the buffer too.
struct SlabSrc {
  const float* slab = nullptr; int splitk = 0; long MN = 0; int N = 0;
  const void* R = nullptr; int ldr = 0;
  void* store = nullptr;
};
struct GNArgs {
  const void* x = nullptr;        // primal input  [Bp][HW][C]
  const void* d = nullptr;        // tangent dx or cotangent gz [NT][HW][C] (modes 1,2)
  void* y = nullptr;              // output (primal y / tangent dz / cotangent gx)
  const float* gamma = nullptr; const float* beta = nullptr;
  int astride = 0;                // row stride of gamma / beta per PRIMAL sample: 0 = one shared affine [C]; C = the per-sample tables of a modulated op (AdaGNTable)
  double* pstats = nullptr;       // [Bp][G][2]  primal (sum, sumsq) -> finalised to (mean, rstd) in place
  double* tstats = nullptr;       // [NT][G][2]  tangent / adjoint sums
  float* part = nullptr;          // per-block partial sums [n][blocks][G][2] (scratch shared by every GroupNorm launch of the stream)
  size_t part_bytes = 0;
  int* ticket = nullptr;          // [n] arrival counters, zero between launches
  int det = 1;                    // 1 (default): bitwise reproducible statistics (fixed-order reductions); 0: atomics (round-1 path, A/B only)
  int red = 0;                    // set by launch_groupnorm: the apply pass adds the statistics launch's per-block partials itself
  int Bp = 1, NT = 0, kps = 1;    // tangent j belongs to primal sample j / kps
  int HW = 0, C = 0, G = 32;
  float eps = 1e-5f;
  int silu = 0, accumulate = 0;
  SlabSrc src;                    // tangent / adjoint, one-launch kernel only: d comes from split-K slabs
};
int launch_groupnorm(int dtype, int mode, const GNArgs& a, hipStream_t st);
// Scale-shift GroupNorm as a per-sample affine: for every modulated op i of the table and sample b < batch
//   og[i][b][c] = gamma[i][c] (1 + s),  ob[i][b][c] = beta[i][c] (1 + s) + h,   (s, h) = emb[i][row][c], emb[i][row][C + c],  row = per_sample ? b : 0
// emb[i]: the op's column window of the fused embedding projection (engine dtype, row pitch ld elements).  fp32 arithmetic.  One launch per
// ADAGN_MAX_OPS ops, the descriptor table in the kernel arguments.
constexpr int ADAGN_MAX_OPS = 32;
struct AdaGNTable { const float* gamma[ADAGN_MAX_OPS]; const float* beta[ADAGN_MAX_OPS]; const void* emb[ADAGN_MAX_OPS]; float* og[ADAGN_MAX_OPS]; float* ob[ADAGN_MAX_OPS]; int C[ADAGN_MAX_OPS]; };
struct AdaGNOp { const float* gamma; const float* beta; const void* emb; float* og; float* ob; int C; };
int launch_adagn_affine(int dtype, const AdaGNOp* ops, int nops, long ld, int batch, int per_sample, hipStream_t st);
bool groupnorm_is_one_launch(int dtype, const GNArgs& a);   // launch_groupnorm runs the one-launch kernel (the one that can take split-K slabs: SlabSrc) for this C, G, HW

struct LNArgs {
  const void* x = nullptr; const void* d = nullptr; void* y = nullptr;
  const float* gamma = nullptr; const float* beta = nullptr;
  int rows_per_sample = 0, Bp = 1, NT = 0, kps = 1, C = 0;
  float eps = 1e-5f;
  int accumulate = 0;
  SlabSrc src;                    // tangent / adjoint: d comes from split-K slabs
};
int launch_layernorm(int dtype, int mode, const LNArgs& a, hipStream_t st);

// ---------------------------------------------------------------- attention pieces
// rows: Z * Lq rows of length ld (valid columns < Lk, the rest are written as 0)
int launch_softmax_fwd(int dtype, void* S, long Z, int Lq, int Lk, int ld, int causal, hipStream_t st);   // causal: query i sees keys <= i
// dP = P o (dS - rowsum(P o dS)), in place on dS; P row index uses z_p = (z / Z2 / kps) * Z2 + z % Z2; optional D out
int launch_softmax_jvp(int dtype, const void* P, void* dS, float* D, long Z, int Z2, int kps, int Lq, int Lk, int ld,
                       hipStream_t st);
// gST[z][j][i] = PT[zp][j][i] * (gPT[z][j][i] - D[z][i])   (in place on gPT)
int launch_softmax_adjT(int dtype, const void* PT, void* gPT, const float* D, long Z, int Z2, int kps, int Lk, int Lq,
                        int ld, hipStream_t st);
// out[z][c][r] = in[z][r][c] for r < R, c < Ccols ; in row stride ldin, in batch strides (s1 over z1, s2 over z2)
int launch_transpose(int dtype, const void* in, void* out, int Z1, int Z2, long s1, long s2, int R, int Ccols, int ldin,
                     int ldout, long outZstride, hipStream_t st);

// fused (flash-style) tangent / adjoint self-attention, bf16, head dim 40 or 80 (attn_fused.hip)
struct FusedAttnArgs {
  const void *Q = nullptr, *K = nullptr, *V = nullptr, *O = nullptr, *KT = nullptr, *VT = nullptr, *QT = nullptr;
  const float* stats = nullptr;
  float* Drow = nullptr;                             // scratch [nt][H][L] floats for the shared-P key-major adjoint (row dots gO . O)
  const void *dQ = nullptr, *dK = nullptr, *dV = nullptr, *dVT = nullptr; void* dO = nullptr;
  const void *gO = nullptr, *gOT = nullptr; void *gQ = nullptr, *gK = nullptr, *gV = nullptr;
  int accQ = 0, accK = 0, accV = 0;
  int fl = 0;                                        // 16-bit flavour: 0 bf16, 1 f16
  int L = 0, C = 0, Co = 0, H = 0, d = 0, kps = 1;   // C: row stride of q/k/v (and their tangents / cotangents), Co: of o
  float scale = 1.f;
};
int fused_attention_supported(int dtype, int d, int L, int kv_const);
void attn_debug_shared(int bits);   // bit 1: shared-P key-major adjoint of the d = 40 layers (default 2; 0 = per-cotangent kernel)
// constant-K/V (cross) attention tangent / adjoint in one launch (attn_fused.hip): Y = c_out [P o (c_in X A^T - delta)] B
struct CrossAttnArgs {
  const void *Q = nullptr, *K = nullptr, *V = nullptr;   // primal q [B][L][C]; k, v [B][Lk][Ck] (column windows allowed)
  const void* BT = nullptr;                              // per-head transpose [B][H][d][Lkp] of V (tangent) or K (adjoint)
  const void* X = nullptr; void* Y = nullptr;            // dQ -> dO (tangent) or gO -> gQ (adjoint)
  int L = 0, Lk = 0, Lkp = 0, C = 0, Ck = 0, Cx = 0, Cy = 0, H = 0, d = 0, kps = 1, adjoint = 0, accumulate = 0, fl = 0;
  int primal = 0;                                        // 1: the forward pass itself, Y = softmax(scale Q K^T) V (X unused; BT may be null: built in LDS)
  float* Pstash = nullptr;                               // primal only: also store the fp32 probabilities [B][L][H][80] (keys >= Lk: zeros) for the folded route (EPI_XATT)
  float scale = 1.f;
};
int cross_attention_supported(int dtype, int d, int Lq, int Lk, int kv_const);
int launch_attn_cross(const CrossAttnArgs& f, int nt, hipStream_t st);
int attn_adj_route_bits(int d, int L, int kps, int nt);   // bit 0: multi-cotangent query-major kernel, bit 1: shared-probability key-major kernel
int attn_jvp_block_waves(int d, int L, int pairs);   // waves per block of the fused tangent kernel launch_attn_jvp_fused picks (pairs = nt * heads)
int launch_attn_fwd_fused(const FusedAttnArgs& f, int batch, void* O, float* stats, hipStream_t st);   // primal O + row statistics
int launch_attn_jvp_fused(const FusedAttnArgs& f, int nt, hipStream_t st);
int launch_attn_adj_fused(const FusedAttnArgs& f, int nt, hipStream_t st);

// ---------------------------------------------------------------- elementwise
struct GegluArgs {
  const void* h = nullptr;     // primal [Bp*rows][2F]
  const void* d = nullptr;     // tangent dh [NT*rows][2F] or cotangent gy [NT*rows][F]
  void* y = nullptr;           // primal y [.. F] / tangent dy [.. F] / cotangent gh [.. 2F]
  int rows_per_sample = 0, Bp = 1, NT = 0, kps = 1, F = 0;
  int accumulate = 0;
  int stash = 1;               // primal: 1 = overwrite (a, g) in h by the factors (G1, G2) the tangent / adjoint passes read; 0 = forward only, h untouched
  int il = 0;                  // 0: h = [a | g] halves; 64: a / g interleaved in blocks of 64 columns (FF-in weight rows repacked, tape.py)
};
int launch_geglu(int dtype, int mode, const GegluArgs& a, hipStream_t st);
int launch_silu(int dtype, const void* x, void* y, long n, hipStream_t st);
int launch_quick_gelu(int dtype, const void* x, void* y, long n, hipStream_t st);   // x * sigmoid(1.702 x) (CLIP ViT-L text encoder MLP)
int launch_gelu(int dtype, const void* x, void* y, long n, hipStream_t st);         // exact erf GELU (OpenCLIP-H text encoder MLP of SD-2.x)
// out[b][c][t] = tok[ids[b][t]][c] + pos[t][c]  (fp32, the engine's NCHW boundary layout with H*W = L tokens); tables in `dtype`
int launch_embed_tokens(int dtype, const int* ids, const void* tok, const void* pos, float* out, int batch, int L, int C, int vocab, hipStream_t st);
int launch_axpy(int dtype, const void* x, void* y, long n, int accumulate, hipStream_t st);   // y (+)= x
// channel concat / split on [rows][C] tensors: copy src[rows][Cs] <-> dst[rows][Cd] column window at c0
int launch_copy_cols(int dtype, const void* src, int lds, int cs0, void* dst, int ldd, int cd0, long rows, int ncols,
                     int accumulate, hipStream_t st);
// dst[rows][ldd] column window [cd0, cd0 + ncols) <- 0
int launch_zero_cols(int dtype, void* dst, int ldd, int cd0, long rows, int ncols, hipStream_t st);
// fp32 NCHW [n][C][HW]  <->  T NHWC [n][HW][Cpad]
int launch_nchw_to_nhwc(int dtype, const float* src, void* dst, int n, int C, int HW, int Cpad, hipStream_t st);
int launch_nhwc_to_nchw(int dtype, const void* src, float* dst, int n, int C, int HW, int Cpad, hipStream_t st);
// h-space shift of a tap, the seam of dpb_forward_shift and dpb_forward_shift_groups: h [groups xb][HW][C] holds samples 0 .. xb-1, and
// h[g xb + b] = h[b] + scale[g xb + b] * u[dir[g xb + b]] in place; (xb, groups) = (1, batch): shifted copies of sample 0, (batch, 1): every row
// shifted where it is.  h: NHWC in the engine dtype (Cv valid channels, the pad channels are copied); u: DEVICE fp32 [nu][Cv][HW] (NCHW-flattened);
// dir / scale: HOST arrays of groups * xb entries (dir in [-1, nu), checked by the caller; -1 = no shift: a copy, or nothing for a row of group 0),
// passed as kernel arguments, SHIFT_MAX_ROWS rows per launch: ceil(xb / floor(SHIFT_MAX_ROWS / groups)) launches, or groups in chunks when there are
// more of them than that.  The sum is formed in fp32 and rounded once; 64-bit offsets; 16-byte accesses on the NHWC side when C is a multiple of the chunk.
constexpr int SHIFT_MAX_ROWS = 64;
struct ShiftRows { int dir[SHIFT_MAX_ROWS]; float scale[SHIFT_MAX_ROWS]; };
int launch_shift_tap(int dtype, void* h, const float* u, const int* dir, const float* scale, int xb, int groups, int C, int Cv, long HW,
                     hipStream_t st);
// sample 0 of each of `nbufs` buffers (sample_bytes[i] bytes per sample, a multiple of 16; 16-byte aligned) copied to samples 1 .. batch-1 in
// place: one launch per REPL_MAX_BUFS buffers, the descriptor table in the kernel arguments, 16-byte copies
constexpr int REPL_MAX_BUFS = 32;
struct ReplTable { void* p[REPL_MAX_BUFS]; long chunks[REPL_MAX_BUFS]; };
int launch_replicate_rows(void* const* bufs, const size_t* sample_bytes, int nbufs, int batch, hipStream_t st);
// 2x2 sum pooling of a cotangent (adjoint of nearest x2 upsampling): in [n][2H*2W][C] -> out [n][H*W][C]
int launch_pool2x2_sum(int dtype, const void* in, void* out, int n, int H, int W, int C, int accumulate, hipStream_t st);
// The two stand-alone 2x2 resampling maps (DPB_OP_RESAMPLE), each the other's adjoint up to the factor; H, W: the SMALL side's size.
//   pool: in [n][2H*2W][C] -> out [n][H*W][C]   (+)= scale * sum of the 2x2 window   (0.25: average pool; 1: adjoint of the upsample)
//   up:   in [n][H*W][C]   -> out [n][2H*2W][C] (+)= scale * in[y/2][x/2]            (1: nearest upsample; 0.25: adjoint of the pool)
// fp32 arithmetic, one rounding; C a multiple of the 16-byte chunk; 64-bit offsets; no atomics.
int launch_pool2x2(int dtype, const void* in, void* out, int n, int H, int W, int C, float scale, int accumulate, hipStream_t st);
int launch_up2x2(int dtype, const void* in, void* out, int n, int H, int W, int C, float scale, int accumulate, hipStream_t st);

// ---------------------------------------------------------------- re-orthonormalisation (fp32 in/out, fp64 Gram)
struct OrthArgs {
  const float* W = nullptr;      // [k][N]  = J^T J V_prev
  const float* Vprev = nullptr;  // [k][N]
  float* V = nullptr;            // [k][N]  right singular vectors of W, rows, descending
  float* s = nullptr;            // [k]     sqrt(singular values of W)   (reference: s.sqrt())
  float* conv = nullptr;         // [2]     {||V - Vprev||_2, max(|V-Vprev| - 1e-5|V|)}
  double* scratch = nullptr;     // >= orth_scratch_bytes(k, N)
  size_t scratch_bytes = 0;
  int k = 0; long N = 0;
  // samples of a batch in ONE set of launches (dpb_pullback_iterate): sample b at W + b*stride_w, Vprev / V + b*stride_v, s + b*stride_s,
  // conv + b*stride_conv (elements), scratch + b*scratch_stride (bytes, a multiple of 8, >= orth_scratch_bytes)
  int batch = 1; long stride_w = 0, stride_v = 0, stride_s = 0, stride_conv = 0; size_t scratch_stride = 0;
};
constexpr int ORTH_MAX_RANK = 128;   // largest pca_rank of the re-orthonormalisation (orth.hip: the k x k fp64 matrix of the eigen-solve lives in LDS)
int launch_orth(const OrthArgs& a, hipStream_t st);
size_t orth_scratch_bytes(int k, long N);

// ---------------------------------------------------------------- randomized low-rank PCA (pca.hip): torch.pca_lowrank(H, q, center=True, niter)
// H [N][D] fp32, R [min(N, D)][q] (torch.randn(A.shape[-1], q) of _svd_lowrank's A), u [q][D] (rows: the reference's u^T), s [q]
const char* pca_invalid(int q, long N, long D);          // nullptr if the shape is supported
size_t pca_scratch_bytes(int q, long N, long D);         // 0 when invalid
int launch_pca_lowrank(const float* H, long N, long D, const float* R, int q, int niter, float* u, float* s, void* scratch, size_t scratch_bytes,
                       hipStream_t st);

// ---------------------------------------------------------------- host-side pieces shared by the geometry launchers (the device pieces: geom.h)
// the parts of a scratch block: take() returns the offset of the next part, each part rounded up to 256 bytes; off is the total so far
struct ScratchCarver {
  size_t off = 0;
  size_t take(size_t bytes) { const size_t o = off; off += (bytes + 255) / 256 * 256; return o; }
};
// a caller's scratch block must be 256-byte aligned and hold `need` bytes; -1 with the error set if not (sizer...: the C-ABI call that returns `need`,
// printf-style, as the message names it)
__attribute__((format(printf, 5, 6))) inline int check_scratch(const char* who, const void* scratch, size_t have, size_t need, const char* sizer, ...) {
  if ((uintptr_t)scratch % 256) { set_error("%s: scratch must be 256-byte aligned", who); return -1; }
  if (have >= need) return 0;
  char call[160];
  va_list ap;
  va_start(ap, sizer);
  vsnprintf(call, sizeof(call), sizer, ap);
  va_end(ap);
  set_error("%s: scratch of %zu bytes, %s = %zu needed", who, have, call, need);
  return -1;
}
// rank classes of the LDS-resident kernels: 16 | 32 | 64 rows, 256 threads for the smallest, 1024 above; DPB_BY_RANK128 adds the 128-row class
#define DPB_BY_RANK(k, ...)                                                \
  do {                                                                     \
    if ((k) <= 16) { constexpr int KM = 16, NT = 256; __VA_ARGS__; }       \
    else if ((k) <= 32) { constexpr int KM = 32, NT = 1024; __VA_ARGS__; } \
    else { constexpr int KM = 64, NT = 1024; __VA_ARGS__; }                \
  } while (0)
#define DPB_BY_RANK128(k, ...)                                             \
  do {                                                                     \
    if ((k) <= 64) DPB_BY_RANK(k, __VA_ARGS__);                            \
    else { constexpr int KM = 128, NT = 1024; __VA_ARGS__; }               \
  } while (0)
// 16-column tiles of the fp64 MFMA kernels: KT = ceil(k / 16) for k <= 64
#define DPB_BY_TILES(k, ...)                                   \
  do {                                                          \
    if ((k) <= 16) { constexpr int KT = 1; __VA_ARGS__; }       \
    else if ((k) <= 32) { constexpr int KT = 2; __VA_ARGS__; }  \
    else if ((k) <= 48) { constexpr int KT = 3; __VA_ARGS__; }  \
    else { constexpr int KT = 4; __VA_ARGS__; }                 \
  } while (0)

// ---------------------------------------------------------------- principal angles between subspaces (angles.hip): exact fp64 cross-Gram on the f64 MFMA,
// then per-basis whitening and a per-pair Jacobi eigen-solve, all fp64.  G [Ra][Rb] fp64; Y = nullptr: Y = X (upper tiles computed, mirrored)
int launch_cross_gram(const float* X, const float* Y, double* G, int Ra, int Rb, long N, hipStream_t st);
size_t subspace_angles_scratch_bytes(long Ba, long Bb, int k, long N);   // 0 when invalid
int launch_subspace_angles(const float* A, const float* B, long Ba, long Bb, int k, long N, float* theta, float* dist, void* scratch, size_t scratch_bytes,
                           hipStream_t st);

// per-basis whitening shared by the angles and the Frechet mean: Dg [n][k][k] fp64 (each basis's own Gram block) -> W = L^-1 D^-1/2 in place (lower
// triangular, W G W^T = I), flags [n] = 1 for a degenerate basis (its slot is then left as it was); one workgroup per basis, k <= ORTH_MAX_RANK
void launch_angles_prep(double* Dg, int* flags, int n, int k, hipStream_t st);
// block b < n of a stacked Gram into its own slot: dst[b][r][c] = G[(b rstep + r) ld + b k + c]   (rstep = k: diagonal blocks; 0: one basis against a stack)
void launch_gram_blocks(const double* G, double* dst, int n, long ld, int rstep, int k, hipStream_t st);
// each basis's own Gram block straight from the rows: Dg[b] [k][k] = X_b X_b^T, X [n][k][N], n <= 65535 (the chains of launch_cross_gram)
int launch_self_gram_blocks(const float* X, double* Dg, int n, int k, long N, hipStream_t st);

// ---------------------------------------------------------------- Frechet (Karcher) mean on the Grassmannian of B bases of k rows (frechet.hip): the
// Riemannian iteration on coefficients against the whitened Gram of all rows; X [B][k][N] fp32, everything between in fp64; see include/dpb.h
constexpr int FRECHET_MAX_RANK = 64;   // three k x k fp64 matrices (S, its eigenvectors, M_i) of the per-basis log map live in LDS
size_t frechet_scratch_bytes(long B, int k, long N, long max_iter);   // 0 when invalid
int launch_frechet_init(const float* X, long B, int k, long N, long max_iter, int init, void* scratch, size_t scratch_bytes, hipStream_t st);
int launch_frechet_iterate(long B, int k, long N, long max_iter, int n_iter, double step, double tol, void* scratch, size_t scratch_bytes, hipStream_t st);
int launch_frechet_finish(const float* X, long B, int k, long N, long max_iter, float* Y, float* weight, float* theta, double* info, void* scratch,
                          size_t scratch_bytes, hipStream_t st);

// the whitened Gram Ghat [R][R] of X with its whitenings W [B][k][k] and flags [B] (dpb_frechet_init's first half), and the streaming finish
// Y [k][N] = Z X from transposed fp64 coefficients Zt [R][k], k <= 64 -- both shared with flagmean.hip
int launch_whitened_gram(const float* X, long B, int k, long N, double* G, double* W, int* flags, hipStream_t st);
int launch_coef_stream(const float* X, const double* Zt, float* Y, int R, int k, long N, hipStream_t st);
const double* frechet_ghat(long B, int k, long N, long max_iter, const void* scratch);   // Ghat inside a Frechet scratch block; nullptr when invalid
int launch_frechet_start(const double* Ct, long B, int k, long N, long max_iter, void* scratch, size_t scratch_bytes, hipStream_t st);

struct FrechetView { const double *G, *W, *Ct, *Rot; const int* flags; size_t total; };
bool frechet_view(long B, int k, long N, long max_iter, void* scratch, FrechetView& v);   // false when invalid

// ---------------------------------------------------------------- principal geodesic analysis of B bases around a base point (pga.hip): the Gram of the log
// maps at the current point of a Frechet scratch block from k x k algebra on Ghat, its (centred) eigen-problem, and the modes in one streaming pass;
// n members = B, or B - 1 when the last basis of the block is the caller's base point; see include/dpb.h
size_t pga_scratch_bytes(long B, long n, int k, long N, int J);   // 0 when invalid
int launch_pga_tangent_gram(long B, long n, int k, long N, long max_iter, int J, void* fscratch, size_t fbytes, double* T, float* theta, int32_t* state,
                            void* scratch, size_t scratch_bytes, hipStream_t st);
int launch_pga_eig(const double* T, long B, long n, int k, long N, int J, int M, int center, double* Wt, double* out, void* scratch, size_t scratch_bytes,
                   hipStream_t st);
int launch_pga_combine(const float* X, const double* Wt, long B, long n, int k, long N, long max_iter, int J, int Jw, void* fscratch, size_t fbytes, float* out,
                       void* scratch, size_t scratch_bytes, hipStream_t st);
void pga_debug_route(int v);   // 0 by size, 1 the one-workgroup Jacobi, 2 the subspace iteration

// ---------------------------------------------------------------- the flag (extrinsic) mean of B bases of k rows (flagmean.hip): the top-r eigenvectors
// of the mean projector by block subspace iteration on the whitened Gram; ghat != nullptr: a caller's Ghat (the scratch then holds the solver only)
constexpr int FLAG_MEAN_MAX_RANK = 64;   // the block of the subspace iteration is at most 64 columns wide: three 64 x 64 fp64 matrices of its head live in LDS
int flag_mean_block_width(long R, int r);
size_t flag_mean_scratch_bytes(long B, int k, long N, int r, long max_iter, bool own);   // 0 when invalid
int launch_flag_mean_init(const float* X, const double* ghat, long B, int k, long N, int r, unsigned long long seed, long max_iter, void* scratch,
                          size_t scratch_bytes, hipStream_t st);
int launch_flag_mean_iterate(const double* ghat, long B, int k, long N, int r, long max_iter, int n_iter, double tol, void* scratch, size_t scratch_bytes,
                             hipStream_t st);
int launch_flag_mean_finish(const float* X, const double* ghat, long B, int k, long N, int r, long max_iter, float* Y, float* weight, float* theta, double* Ct,
                            double* info, void* scratch, size_t scratch_bytes, hipStream_t st);
// the weighted flag mean (zero rounds) and the flag median by iteratively reweighted flag means (flagmean.hip): the same solver on D Ghat D, a round
// per reweighting; member_weight [B] fp64 on the device or nullptr (uniform); member [3][B]: affinity, distance, member weight
size_t flag_median_scratch_bytes(long B, int k, long N, int r, long max_iter, bool own);   // 0 when invalid
int launch_flag_median_init(const float* X, const double* ghat, const double* member_weight, long B, int k, long N, int r, unsigned long long seed, long max_iter,
                            void* scratch, size_t scratch_bytes, hipStream_t st);
int launch_flag_median_iterate(const double* ghat, long B, int k, long N, int r, long max_iter, int n_iter, double tol, void* scratch, size_t scratch_bytes,
                               hipStream_t st);
int launch_flag_median_round(const double* ghat, long B, int k, long N, int r, long max_iter, double eps, double tol, int update, void* scratch,
                             size_t scratch_bytes, hipStream_t st);
int launch_flag_median_finish(const float* X, const double* ghat, long B, int k, long N, int r, long max_iter, float* Y, float* weight, float* theta, double* Ct,
                              double* member, double* info, void* scratch, size_t scratch_bytes, hipStream_t st);

// ---------------------------------------------------------------- flag k-means and the chordal affinity of two stacks (flagkmeans.hip): Lloyd's
// algorithm with flag-mean centres on coefficients against the whitened Gram; the caller owns the rounds and runs the flag-mean solver per cluster
size_t flag_affinity_scratch_bytes(long Ba, int k, long Bc, int r, long N);   // 0 when invalid
int launch_flag_affinity(const float* A, const float* Y, long Ba, int k, long Bc, int r, long N, double* aff, void* scratch, size_t scratch_bytes,
                         hipStream_t st);
size_t flag_kmeans_scratch_bytes(long B, int k, long N, long C, int r);       // 0 when invalid
size_t flag_kmeans_host_bytes(long B, int k, long N, long C, int r);          // the leading part of the block the caller reads; 0 when invalid
const double* flag_kmeans_affinity(long B, int k, long N, long C, int r, const void* scratch);   // a [B][C] inside the block; nullptr when invalid
int launch_flag_kmeans_init(const float* X, long B, int k, long N, long C, int r, const int32_t* seeds, int n_seeds, void* scratch, size_t scratch_bytes,
                            hipStream_t st);
int launch_flag_kmeans_gather(long B, int k, long N, long C, int r, int c, int n_c, double* Gc, void* scratch, size_t scratch_bytes, hipStream_t st);
int launch_flag_kmeans_set_centre(long B, int k, long N, long C, int r, int c, int n_c, const double* Ct, void* scratch, size_t scratch_bytes, hipStream_t st);
int launch_flag_kmeans_assign(long B, int k, long N, long C, int r, int apply, void* scratch, size_t scratch_bytes, hipStream_t st);
int launch_flag_kmeans_finish(const float* X, long B, int k, long N, long C, int r, float* Y, void* scratch, size_t scratch_bytes, hipStream_t st);

// ---------------------------------------------------------------- the Hungarian-matched mean of B bases of k rows (hungarian.hip): a batched
// linear-assignment solver (shortest augmenting paths in LDS, one workgroup per problem) and a streaming mean of permuted, signed rows; see include/dpb.h
constexpr int HUNGARIAN_MAX_RANK = 128;   // the k x k fp64 cost matrix lives in LDS: 128 KiB of the 160 KiB a workgroup may declare
size_t linear_assignment_scratch_bytes(long B, int k);   // 0 when invalid
int launch_linear_assignment(const double* cost, long B, int k, int32_t* col_of_row, double* total, void* scratch, size_t scratch_bytes, hipStream_t st);
size_t matched_mean_scratch_bytes(long B, int k, long N);   // 0 when invalid
int launch_matched_mean(const float* X, long B, int k, long N, const float* anchor, int init, int distance, float* Y, int32_t* perm, int32_t* sign,
                        double* info, void* scratch, size_t scratch_bytes, hipStream_t st);

// ---------------------------------------------------------------- parallel transport of directions between tangent spaces (transport.hip)
// vk[d][p] = normalise(sum_q c[d][p][q] vhat_dst[d][q]), c[d][p][q] = <uhat_dst[d][q], uhat_src[pcs[p]]> (fp64), coef_norm = ||c||; pcs is a HOST list
size_t transport_scratch_bytes(long D, int P, int k, long Nh, long Nx);   // 0 when invalid
// ss[r] = sum_n X[r][n]^2 in fp64, the fixed-order reduction of the transport kernel (a chain that depends on N only); X [rows][N] fp32
int launch_rowsumsq(const float* X, long rows, long N, double* ss, hipStream_t st);
int launch_transport_directions(const float* u_src, const float* u_dst, const float* vT_dst, const int32_t* pcs, int P, long D, int k, long Nh, long Nx,
                                float* vk, float* coef, float* coef_norm, void* scratch, size_t scratch_bytes, hipStream_t st);

// ---------------------------------------------------------------- the perturbed batch of local PCA (noise.hip)
// out[b][j] = x[j] + norm * g_b[j] / ||g_b||_2, b < B, j < n (fp32); g_b = noise[b] or Philox4x32-10 normals of (seed, first + b) (dpb.h);
// noise_out (optional) receives the unnormalised g; scratch: 8-byte aligned, >= perturb_scratch_bytes(B, n) (per-slice fp64 partial sums)
size_t perturb_scratch_bytes(int B, long n);             // 0 when invalid
int launch_perturb_unit(const float* x, const float* noise, uint64_t seed, int64_t first, int B, long n, float norm, float* out, float* noise_out,
                        void* scratch, size_t scratch_bytes, hipStream_t st);

// ---------------------------------------------------------------- the parallel-h edit chain (chain.hip): what lies between the U-Net passes of a step
// direction step: W = J^T c [n][N] -> v = -W / ||W|| (fp64, rounded once), the SEGA mask (sega_sigma <= 0: off), x_out = x + step[b] v (x_out may alias
// x; vk optional), stats [n][4] fp64 on the device = (sum w^2, std or 0, elements kept, flag); step: a HOST array; see include/dpb.h
constexpr int CHAIN_MAX_ROWS = 256;       // rows per launch: the host lists (step; dir and sign) travel as kernel arguments
size_t direction_step_scratch_bytes(long n, long N);     // 0 when invalid
int launch_direction_step(const float* W, const float* x, float* x_out, float* vk, const float* step, float sega_sigma, long n, long N, double* stats,
                          void* scratch, size_t scratch_bytes, hipStream_t st);
// out [n][2] fp64 = (<h - h0, c> / ||c||, ||h - h0||^2), c = sign[b] u[dir[b]]; u [nu][D] on the device, dir / sign HOST arrays (validated here)
int launch_shift_stats(const float* h, const float* h0, const float* u, int nu, const int32_t* dir, const float* sign, long n, long D, double* out,
                       hipStream_t st);
// cot[b] = sign[b] u[dir[b]]: the chain's cotangents, one per sample
int launch_gather_cotangents(const float* u, int nu, const int32_t* dir, const float* sign, long n, long D, float* cot, hipStream_t st);

// ---------------------------------------------------------------- the h-space guidance edit (hguide.hip)
// the asymmetric DDIM step: d = e_s - e, eP = e + gP d, eD = e + gD d, out = sqrt(a_next) (x - eP sqrt(1-a_t)) / sqrt(a_t) + sqrt(1-a_next) eD in the
// operation order of ddim_kernel (out may alias x; x0 optional: the predicted x0); stats [n][2] fp64 on the device = (sum d^2, flag); see include/dpb.h
size_t ddim_step_asym_scratch_bytes(long n, long N);     // 0 when invalid
int launch_ddim_step_asym(const float* x, const float* e, const float* es, float* out, float* x0, long n, long N, float a_t, float a_next, float gP,
                          float gD, double* stats, void* scratch, size_t scratch_bytes, hipStream_t st);
// ---------------------------------------------------------------- pullback geodesics between two latents (geodesic_chain.hip)
// a curve of m + 2 rows, the end rows fixed.  cotangents: h [m+2][D] -> cot [m][D] = fl32(2 h_i - h_{i-1} - h_{i+1}), seg [m+1] fp64 =
// ||h_{i+1} - h_i||^2, csq [m] fp64 (optional) = ||cot_i||^2.  update: P_out_i = fl32(P_i - eta (W_i + lambda (2 P_i - P_{i-1} - P_{i+1}))), end rows
// copied (P_out must not overlap P), stats [m][4] fp64 = (sum W^2, sum g^2, sum (P_out - P)^2, flag), xseg [m+1] fp64 of the OLD curve; see include/dpb.h
size_t geodesic_cotangents_scratch_bytes(long m, long D);   // 0 when invalid
int launch_geodesic_cotangents(const float* h, float* cot, double* seg, double* csq, long m, long D, void* scratch, size_t scratch_bytes, hipStream_t st);
size_t geodesic_update_scratch_bytes(long m, long N);       // 0 when invalid
int launch_geodesic_update(const float* P, const float* W, float* P_out, float eta, float lambda, long m, long N, double* stats, double* xseg,
                           void* scratch, size_t scratch_bytes, hipStream_t st);
// ---------------------------------------------------------------- the least-squares inverse of the Jacobian (cgls.hip): CGLS between the passes
// R independent rows of min ||J d - c||^2 + mu ||d||^2; d, p, w [R][N], r, q, c [R][D] fp32; state [R][8] and hist [R][4] fp64 on the device;
// d, r and p are updated in place; one scratch size for the three steps; see include/dpb.h
size_t cgls_scratch_bytes(long R, long N, long D);          // 0 when invalid
int launch_cgls_init(const float* c, const float* w0, float* delta, float* r, float* p, double* state, double* hist, double mu_abs, double mu_rel,
                     double tol, long R, long N, long D, void* scratch, size_t scratch_bytes, hipStream_t st);
int launch_cgls_h_step(const float* q, float* delta, float* r, float* p, double* state, double* hist, long R, long N, long D, void* scratch,
                       size_t scratch_bytes, hipStream_t st);
int launch_cgls_x_step(const float* w, float* delta, float* r, float* p, double* state, double* hist, double tol, long R, long N, long D, void* scratch,
                       size_t scratch_bytes, hipStream_t st);
// the newton-h chain around an inner solve: res = fl32(h0 + frac scale[b] sign[b] u[dir[b]] - h) (dir / sign / scale HOST arrays), and
// x_out = fl32(x + kappa d), kappa = min(1, radius / ||d||) with ||d||^2 from the solver's state, step_stats [n][4] = (||res||^2, ||d||^2, kappa, flag)
int launch_newton_residual(const float* h0, const float* h, const float* u, int nu, const int32_t* dir, const float* sign, const float* scale,
                           double frac, long n, long D, float* res, hipStream_t st);
int launch_newton_update(const float* x, const float* delta, const double* state, double radius, float* x_out, double* step_stats, long n, long N,
                         hipStream_t st);
// ---------------------------------------------------------------- DDIM
// x_next =sqrt(a_next) * (x - e*sqrt(1-a_t))/sqrt(a_t) + sqrt(1-a_next) * e      (fp32, elementwise)
int launch_ddim_step(const float* x, const float* e, float* out, float* x0, long n, float a_t, float a_next, hipStream_t st);
// out = a*x + b*y + c*z (z may be null)
int launch_lincomb(const float* x, const float* y, const float* z, float* out, long n, float a, float b, float c, hipStream_t st);

}  // namespace dpb
