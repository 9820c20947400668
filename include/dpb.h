/* dpb.h -- C ABI of the MI355X-native pullback engine (libdpb.so, gfx950).
 *
 * Drop-in boundary for ONE path of enkeejunior1/Diffusion-Pullback: the power-iteration
 * low-rank SVD of the U-Net latent->feature Jacobian and the U-Net forwards of the DDIM loop.
 * The reference has no FFI (it is pure Python over diffusers); its boundary is Python method
 * injection onto the U-Net object (reference src/utils/utils.py:103-104, :326-337).  The host
 * shim diffusion_pullback_amd/ re-creates those methods on top of the entry points below;
 * INTEGRATION.md shows the binding a maintainer would add.  Each entry point cites the
 * reference code it replaces.
 *
 * Conventions: plain pointers and sizes, no torch types.  All tensor pointers are DEVICE
 * pointers unless marked host.  Every call enqueues work on the engine's stream
 * (dpb_engine_set_stream; default stream 0) and returns without synchronising unless stated.
 * Return value: 0 = success, nonzero = failure (message via dpb_last_error()).  One engine per
 * GPU per process; calls on one engine must not overlap (thread-compatible, not thread-safe).
 * The engine never allocates device memory: the caller sizes (dpb_engine_workspace_bytes) and
 * provides (dpb_engine_set_workspace) one zero-initialisable workspace, and owns the weights.
 */
#ifndef DPB_H
#define DPB_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPB_ABI_VERSION 1

enum { DPB_F32 = 0, DPB_BF16 = 1, DPB_F16 = 2 };   /* storage + MFMA input type; accumulation is always fp32 */

/* ---- network description: a tape of NHWC ops over numbered activation buffers ------------- */
enum {
  DPB_OP_CONV = 1,      /* conv KSxKS / 1x1 / Linear: out = W*in (+bias) (+rowbias[temb]) (+res)      */
  DPB_OP_GROUPNORM = 2, /* GroupNorm(G, eps) (+SiLU); optionally modulated per sample: (gamma x^ + beta)(1 + scale_b) + shift_b,
                           (scale_b | shift_b) a 2C-wide column window of the SHARED buffer in1 (see dpb_op_desc)          */
  DPB_OP_LAYERNORM = 3, /* LayerNorm over channels                                                     */
  DPB_OP_ATTENTION = 4, /* multi-head softmax(q k^T d^-1/2) v ; in0=q in1=k in2=v                      */
  DPB_OP_GEGLU = 5,     /* [rows][2F] -> [rows][F] : a * gelu_erf(g).  dpb_primal OVERWRITES the input buffer
                           by the factors (gelu(g), a*gelu'(g)) its tangent / adjoint passes read: the input must
                           have no other consumer (checked at create) and is not a meaningful tap afterwards;
                           dpb_forward leaves it untouched                                              */
  DPB_OP_SILU = 6,      /* elementwise x*sigmoid(x); ip[0] = 1: quick-GELU x*sigmoid(1.702x), 2: erf GELU (primal only) */
  DPB_OP_CONCAT = 7,    /* channel concat of in0, in1                                                  */
  DPB_OP_RESAMPLE = 8   /* stand-alone 2x2 resampling of an NHWC map, C unchanged: ip[0] = 0 average pool (H x W -> H/2 x W/2, H and W even),
                           ip[0] = 1 nearest x2 upsample (H x W -> 2H x 2W); ip[1], ip[2] = input H, W.  The h_upd / x_upd of the guided-diffusion
                           ResBlock with up / down (reference src/models/guided_diffusion/unet.py:192-197, :239-244: Downsample / Upsample with
                           use_conv = False, i.e. avg_pool2d(2) and F.interpolate(scale_factor=2, mode="nearest")).  Tangent: the same map;
                           adjoint of the pool: 0.25 x nearest upsample, of the upsample: the 2x2 sum.  fp32 arithmetic, one rounding    */
};
enum { DPB_GATHER_NONE = 0, DPB_GATHER_CONV = 1, DPB_GATHER_UPCONV = 3 };
enum { DPB_BUF_ACT = 0,     /* per-sample activation [rows][channels]                                   */
       DPB_BUF_SHARED = 1   /* independent of x (time-embedding path): one copy shared by the batch, or one
                               row per sample when the samples' timesteps differ (dpb_primal_t)          */ };

typedef struct dpb_buffer_desc {
  int32_t rows;       /* H*W or token count, per sample */
  int32_t channels;   /* stored channel count (multiple of 8) */
  int32_t kind;       /* DPB_BUF_* */
  int32_t valid_channels; /* un-padded channel count seen at the fp32 NCHW boundary; 0 = channels */
} dpb_buffer_desc;

typedef struct dpb_op_desc {
  int32_t kind;              /* DPB_OP_* */
  int32_t in0, in1, in2;     /* input buffer ids, -1 = none */
  int32_t out;               /* output buffer id */
  int32_t res;               /* CONV: buffer added to the output (residual / shortcut), -1 = none */
  int32_t rowbias;           /* CONV: DPB_BUF_SHARED buffer [1][>= Cout] added to every row (temb projection; dpb_primal_t: sample b's row to sample b's rows), -1 */
  int32_t ip[12];            /* CONV: H W Cin Ho Wo Cout KS stride pad gather rowbias_col (first column of this op's Cout-wide window in the rowbias buffer) ; GROUPNORM: G silu modulated mod_col ;
                                ATTENTION: heads oq ok ov causal ; GEGLU: F interleave(0|64) ; RESAMPLE: mode(0 pool | 1 up) H W
                                GROUPNORM with ip[2] = 1 (scale-shift norm, "AdaGN": out_norm(h) * (1 + scale) + shift, unet.py:250-254): in1 is the
                                DPB_BUF_SHARED buffer of the ResBlocks' fused embedding projection (produced by an op), ip[3] the first column of this
                                op's `scale` window [C]; `shift` follows at ip[3] + C.  The primal / forward pass folds both into a per-sample affine
                                gamma_b = gamma (1 + scale_b), beta_b = beta (1 + scale_b) + shift_b (fp32 tables in the workspace, filled right
                                after the projection; row b of the projection under dpb_primal_t, row 0 otherwise); scale and shift do not depend on x,
                                so the tangent / adjoint formulas are those of the plain op with gamma_b.  ip[2] = 0 (in1 ignored, -1): the plain op */
  float fp[4];               /* GROUPNORM/LAYERNORM: eps */
  const void* w[4];          /* CONV: w[0]=W [Cout][KS*KS*Cin] (engine dtype), w[1]=W^T [Cin][KS*KS*Cout]
                                (engine dtype, for the adjoint; may be NULL for ops never differentiated),
                                w[2]=bias fp32 [Cout] or NULL ; norms: w[0]=gamma fp32, w[1]=beta fp32   */
} dpb_op_desc;

typedef struct dpb_net_desc {
  int32_t dtype;             /* DPB_F32 | DPB_BF16 | DPB_F16 */
  int32_t max_batch;         /* max primal samples per call */
  int32_t max_tangents;      /* max total tangents/cotangents per call (k * samples) */
  int32_t n_buffers, n_ops;
  const dpb_buffer_desc* buffers;
  const dpb_op_desc* ops;
  int32_t x_buf;             /* input buffer (NHWC, channels padded); x_channels true channels */
  int32_t x_channels;
  int32_t temb_buf;          /* DPB_BUF_SHARED [1][temb_dim] sinusoid input, -1 = none */
  int32_t temb_dim;
  int32_t temb_flip_sin_to_cos;   /* 1: [cos|sin] (diffusers SD), 0: [sin|cos] (DDPM) */
  int32_t temb_half_minus_one;    /* 1: exponent denominator half_dim-1 (DDPM), 0: half_dim (SD) */
  int32_t ctx_buf;           /* per-sample conditioning buffer [ctx_len][ctx_dim], -1 = none */
} dpb_net_desc;

typedef struct dpb_engine dpb_engine;

const char* dpb_last_error(void);
int dpb_abi_version(void);

/* Build the executor for a network.  Weight pointers in `net` must stay valid for the engine's life.
 * Replaces: the diffusers U-Net module tree the reference walks in get_h (utils.py:438-527, :114-163). */
int dpb_engine_create(const dpb_net_desc* net, dpb_engine** out);
void dpb_engine_destroy(dpb_engine* e);
int dpb_engine_set_stream(dpb_engine* e, void* hip_stream);
size_t dpb_engine_workspace_bytes(const dpb_engine* e);
/* `ws` must be 256-byte aligned device memory of at least workspace_bytes; it is zero-filled here. */
int dpb_engine_set_workspace(dpb_engine* e, void* ws, size_t bytes);

/* Primal pass: run ops up to (and including) the producer of `upto_buf`, keeping every activation
 * and normalisation statistic resident for the tangent/adjoint passes.
 * x: fp32 NCHW [batch][x_channels][rows(x_buf)], t: timestep (host float, shared by the batch),
 * ctx: fp32 [batch][ctx_len][ctx_dim] or NULL.
 * Replaces: unet.get_h(...) / unet(x, t, encoder_hidden_states) (utils.py:438-527; edit.py:454-458). */
int dpb_primal(dpb_engine* e, const float* x, int batch, float t, const float* ctx, int upto_buf);
/* Forward only (the U-Net calls of the DDIM / guidance loop, edit.py:454-458, :484-502): the same pass without the tangent / adjoint
 * stash (no K^T / Q^T / P^T copies, GEGLU inputs left untouched), result copied to `out` as fp32 NCHW [batch][channels][rows(upto_buf)].
 * Invalidates the engine's primal state: dpb_jvp / dpb_vjp / dpb_pullback_iterate fail until the next dpb_primal. */
int dpb_forward(dpb_engine* e, const float* x, int batch, float t, const float* ctx, int upto_buf, int channels, float* out);
/* Per-sample timesteps (additive to ABI version 1): dpb_primal / dpb_forward with t a HOST array of `batch` entries.  Row b of every activation is
 * the net at (x_b, t[b], ctx_b) -- the ordinary batched U-Net call unet(sample, timestep = tensor([t0, t1, ...]), ...), and the batch of the
 * reference's local-tangent-space job whose rows differ only in t (fix_xt; src/modules/edit.py:1517-1599).  When all entries are equal the call IS
 * the scalar entry point: same launches, same bits.  Otherwise the x-independent chain (sinusoid, the time-embedding linears, SiLU, the fused
 * time_emb_proj product) runs once per sample, with the launches of a scalar call, into that sample's row of the DPB_BUF_SHARED buffers (each has
 * max_batch rows in the workspace), and every ResBlock product reads its row bias at row sample(m): sample b's bias row has the bits of a scalar
 * call at t[b], and an activation row the bits of the same batch run at the scalar t[b].  A few small launches per sample, in the primal only:
 * dpb_jvp / dpb_vjp / dpb_pullback_iterate, the *_between passes and dpb_read_buffer read the stash and work unchanged (dpb_read_buffer of a SHARED
 * buffer returns sample 0's row).  No device allocation; one host synchronisation, as dpb_primal.  dpb_forward_from, dpb_forward_shift and
 * dpb_local_pca_sample take one t for their batch.
 * Refused (dpb_last_error): null t, batch outside [1, max_batch], a non-finite t[b]; distinct timesteps on a network without a timestep
 * embedding (temb_buf = -1, or a temb_buf that no op reads: the VAE and text-encoder tapes only fill the slot) or on a tape where something other than a SHARED op (a Linear or an activation writing a
 * SHARED buffer) or a row bias reads a SHARED buffer (found at dpb_engine_create, the message names the op). */
int dpb_primal_t(dpb_engine* e, const float* x, int batch, const float* t /*host [batch]*/, const float* ctx, int upto_buf);
int dpb_forward_t(dpb_engine* e, const float* x, int batch, const float* t /*host [batch]*/, const float* ctx, int upto_buf, int channels, float* out);
/* Copy a primal activation out as fp32 NCHW [batch][channels][rows] (first `channels` channels). */
int dpb_read_buffer(dpb_engine* e, int buf, int channels, float* out);

/* U = J V : forward-mode pass of `nt` tangents through the same kernels (nt = batch * tangents per
 * sample, tangent j belongs to sample j / (nt/batch)).  V fp32 NCHW [nt][x_channels][rows(x)],
 * U fp32 NCHW [nt][channels(tap)][rows(tap)].   Replaces: torch.func.jacfwd block, utils.py:766-775. */
int dpb_jvp(dpb_engine* e, int tap_buf, const float* V, int nt, float* U);
/* W = J^T U : adjoint pass wrt the input only.  Replaces: autograd.functional.jacobian, utils.py:790-797. */
int dpb_vjp(dpb_engine* e, int tap_buf, const float* U, int nt, float* W);

/* Thin SVD of W [k][N] (fp32, k <= 128): V rows = right singular vectors (descending), s = sqrt(singular values),
 * conv[0] = ||V - Vprev||_2, conv[1] = max(|V - Vprev| - 1e-5|V|).  scratch: device memory of >= dpb_orth_scratch_bytes(k, N) bytes (Gram
 * matrix and distance partials per block, added in block order: the result is bitwise reproducible).  V may alias Vprev (in place:
 * every element of Vprev is read by the thread that overwrites it, after the Gram pass has finished with it).
 * Domain: this is the Gram method (eigen-decomposition of W W^T in fp64), which squares the condition number: V and s have full fp32 accuracy up
 * to cond(W) ~ 1e4; beyond that the trailing vectors degrade (tests/test_gpu_orth.py).  Rows of W that are exactly orthogonal to all
 * others are not mixed; equal singular values among them come out in input order.
 * Non-finite input (tests/test_gpu_orth.py):
 *   - a NaN or an inf anywhere in W: every element of V and of s is NaN and conv = (NaN, NaN); the call returns 0.  The eigen-solve is skipped (the
 *     Gram diagonal sum w^2 tells) and no index derived from data leaves [0, k): the eigenvalue ranking is a total order (NaN first).
 *   - W finite, a NaN or an inf in Vprev: s is bitwise that of the call with a finite Vprev, every row of V is bitwise plus or minus that call's row
 *     (only the sign alignment reads Vprev), and conv = (NaN, NaN).
 *   - conv[0] and conv[1] both propagate a NaN through every reduction; neither is ever inf for a non-finite input.
 *   The next call on the same scratch is unaffected (the scratch carries nothing from call to call).
 * Replaces: torch.linalg.svd + dist/allclose inputs, utils.py:799-806.  Engine-independent. */
int dpb_orth(const float* W, const float* Vprev, float* V, float* s, float* conv, void* scratch, int k, int64_t N,
             void* hip_stream);
size_t dpb_orth_scratch_bytes(int k, int64_t N);   /* 0 for k outside [1, 128] */
/* The same with the caller's scratch size stated and validated.  CONTRACT CHANGE of round 3, called out here because dpb_orth cannot check it: the
 * scratch grew from 8 (3 k^2 + 2) bytes to dpb_orth_scratch_bytes(k, N) (per-block partials of the fixed-order reductions, up to ~129 k^2 + 512
 * doubles); a caller that still sizes it by the old rule gets out-of-bounds device writes from dpb_orth.  New callers bind THIS entry point
 * (the in-repo shim does): it fails with a message instead. */
int dpb_orth_checked(const float* W, const float* Vprev, float* V, float* s, float* conv, void* scratch, size_t scratch_bytes, int k, int64_t N,
                     void* hip_stream);

/* ---- randomized low-rank PCA of a feature matrix (additive to ABI version 1; engine-independent) ------------------------------
 * torch.pca_lowrank(H, q, center=True, niter) -- torch._lowrank._svd_lowrank + get_approximate_basis (Halko et al. 2009, 4.4 / 5.1) -- of
 * H [N][D] fp32 (N samples of D features), as the reference's global_pca_zt calls it (src/utils/utils.py:978-1027, the pca_lowrank at :1017).
 * R: the Gaussian draw of get_approximate_basis exactly as torch.randn(A.shape[-1], q) makes it for _svd_lowrank's A: [N][q] if N < D
 * (A = H^T), else [D][q].  Out: u [q][D] (rows = the columns of the reference's u = _svd_lowrank's V, sign arbitrary), s [q] (its S,
 * descending).  The QR factorisations and svd(B) are dpb_orth (same spans); products on the f32-input MFMA, every reduction in a fixed
 * order (bitwise reproducible), 64-bit offsets (H may exceed 4 GiB).  1 <= q <= 128, q <= N - 1, q <= D, niter >= 0; scratch: device
 * memory of >= dpb_pca_scratch_bytes(q, N, D) bytes (any alignment).  No host synchronisation.  A rank-deficient centred H gives s = 0
 * in the missing directions (and zero rows of u).  A NaN or an inf anywhere in H or R: every element of u and of s is NaN and the call returns 0
 * (the rule of dpb_orth, which every factorisation goes through); the next call on the same scratch is unaffected.  Errors via dpb_last_error. */
size_t dpb_pca_scratch_bytes(int q, int64_t N, int64_t D);   /* 0 when invalid */
int dpb_pca_lowrank(const float* H, int64_t N, int64_t D, const float* R, int q, int niter, float* u, float* s, void* scratch,
                    size_t scratch_bytes, void* hip_stream);

/* ---- local h-space PCA: the perturbed batch and the sampling loop (additive to ABI version 1) ---------------------------------------
 * out[b][j] = x[j] + norm * g_b[j] / ||g_b||_2 for b < B, j < n, all fp32: B unit-norm (norm = 1) perturbations of ONE input, the
 * reference's x + normalize_wrt_batch(torch.randn_like(x)) (src/utils/utils.py:918-925; src/models/ddpm/diffusion.py:399-401).  Engine-independent.
 * g_b is noise[b] when `noise` is given ([B][n], unnormalised Gaussian draws), else it is generated in the kernel, a function of
 * (seed, first + b) only -- not of B, of the chunking or of the launch:
 *   Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11; multipliers D2511F53 / CD9E8D57, Weyl constants 9E3779B9 / BB67AE85), key =
 *   (seed & 0xffffffff, seed >> 32), counter = (i & 0xffffffff, i >> 32, c & 0xffffffff, c >> 32) with i = first + b the 64-bit sample
 *   index and c = j / 4 the index of the group of four elements; the output words (w0, w1, w2, w3) give the elements 4c .. 4c+3:
 *     u(w) = ((w >> 9) + 0.5) * 2^-23      an odd multiple of 2^-24 in (0, 1): 24 significant bits, so exact in fp32, never 0, never 1
 *                                          (the 24-bit variant ((w >> 8) + 0.5) * 2^-24 needs 25 bits and would round)
 *     g[4c]   = sqrt(-2 ln u(w0)) cos(2 pi u(w1))      g[4c+1] = sqrt(-2 ln u(w0)) sin(2 pi u(w1))
 *     g[4c+2] = sqrt(-2 ln u(w2)) cos(2 pi u(w3))      g[4c+3] = sqrt(-2 ln u(w2)) sin(2 pi u(w3))        (fp32 arithmetic)
 * ||g_b||^2 is summed in fp64 in a fixed order (partial sums of slices of 4096 elements, then the slices in index order; no atomics), the
 * factor norm / ||g_b|| is rounded to fp32 once and applied by one fused multiply-add per element: bitwise reproducible, and sample i's row
 * does not depend on B or `first`.  noise_out (optional) receives the unnormalised g.  1 <= B <= 65535, n >= 1 (any n; 16-byte accesses
 * when n % 4 == 0 and the pointers are 16-byte aligned), 0 <= first; scratch: 8-byte aligned device memory of >= dpb_perturb_scratch_bytes(B, n)
 * bytes.  out must not alias x or noise.  No host synchronisation.  Errors via dpb_last_error. */
size_t dpb_perturb_scratch_bytes(int B, int64_t n);   /* 0 when invalid */
int dpb_perturb_unit(const float* x, const float* noise /*[B][n] or NULL*/, uint64_t seed, int64_t first, int B, int64_t n,
                     float norm, float* out /*[B][n]*/, float* noise_out /*[B][n] or NULL: the unnormalised g*/,
                     void* scratch, size_t scratch_bytes, void* hip_stream);
/* The sampling loop of local_pca_zt / local_pca_xt (src/utils/utils.py:916-933; src/models/ddpm/diffusion.py:396-409): rows first .. first + count - 1
 * of the feature matrix, H[i] = get_h(x + g_i / ||g_i||) at the tap upto_buf (fp32 NCHW-flattened, D = channels * rows(upto_buf)).  `H` points at
 * the row of sample `first`, `noise` (or NULL: generated from (seed, sample index) as above) at its noise row.  x [1][N_in] is ONE input, ctx
 * [1][L][Dc] ONE conditioning (or NULL for a network without), both repeated on the device.  The samples go through in chunks of the engine's
 * max_batch: dpb_perturb_unit into scratch, then the dpb_forward pass with the features written straight into their rows of H.  The engine
 * workspace does not grow: scratch is 256-byte aligned device memory of >= dpb_local_pca_scratch_bytes(e) bytes (the perturbed chunk, max_batch
 * copies of ctx, the norm partials).  Host synchronisation: none per chunk; the one upload of the timestep embedding that every dpb_forward makes
 * happens once per call (the chunks share t).  State rules and error paths of dpb_forward: no primal state afterwards, errors via
 * dpb_last_error. */
size_t dpb_local_pca_scratch_bytes(const dpb_engine* e);
int dpb_local_pca_sample(dpb_engine* e, const float* x /*[1][N_in]*/, float t, const float* ctx /*[1][L][Dc] or NULL*/,
                         int upto_buf, int channels, const float* noise /*[count][N_in] or NULL*/, uint64_t seed,
                         int64_t first, int64_t count, float* H /*[count][D] rows first.. of the caller's matrix*/,
                         void* scratch, size_t scratch_bytes);

/* ---- principal angles and geodesic distances between subspaces (additive to ABI version 1; engine-independent) ------------------------
 * The analysis the bases (u, s, vT) of run_sample_encoder_local_tangent_space_zt are saved for (src/modules/edit.py:310-383, :1517-1599; the
 * reference has no code for it): the principal angles theta_1..theta_k between two k-dimensional subspaces of R^N and the geodesic distance
 * ||theta||_2 on the Grassmannian.  Distances only (transport of directions: the next section; the Frechet mean: the one after).
 *
 * dpb_cross_gram: G[i][j] = sum_n X[i][n] Y[j][n].  X [Ra][N], Y [Rb][N] fp32, G [Ra][Rb] FP64 (row stride Rb).  The fp32 inputs are widened on
 * load and multiplied on the fp64 matrix cores (v_mfma_f64_16x16x4_f64), so every product is exact and only the fp64 accumulation rounds.  Y = NULL
 * means Y = X (Rb must equal Ra): only the 64 x 64 tiles on and above the diagonal are computed, the others are their mirror images (G is exactly
 * symmetric).  N is cut into at most eight slices whose length depends on N only; the slices are added into G in slice order by stream-ordered
 * launches, no atomics: bitwise reproducible, and an entry does not depend on Ra, Rb or its position.  Ra, Rb, N >= 1 (Ra <= 4 194 240), any N
 * (16-byte loads when N % 4 == 0 and X, Y are 16-byte aligned), 64-bit offsets (X may exceed 4 GiB).  G must not alias X or Y.  No scratch, no device
 * allocation, no host synchronisation.
 *
 * dpb_subspace_angles: A [Ba][k][N], B [Bb][k][N] fp32, stacks of bases, one basis per k rows; the rows need NOT be orthonormal (u is J V_prev,
 * un-normalised) but must be linearly independent.  theta [Ba][Bb][k] fp32, descending per pair (the convention of scipy.linalg.subspace_angles),
 * dist [Ba][Bb] fp32 = ||theta||_2 (summed in fp64).  Method, everything after the inputs in fp64: the cross-Gram of all rows as above (one pass
 * over A and B; nothing of size N is orthonormalised or written); per basis the rows are normalised through the Gram diagonal and the basis is
 * whitened by the Cholesky factor of its own block, Ghat_ii = L_i L_i^T; per pair M = L_i^-1 Ghat_ij L_j^-T, the eigenvalues l of S = I - M M^T
 * (two-sided Jacobi, in LDS) clamped to [0, 1], theta = asin(sqrt(l)) for l <= 1/2, else acos(sqrt(1 - l)).  Measured against
 * scipy.linalg.subspace_angles in float64 on the same fp32 inputs: <= 1e-6 rad per angle for bases of condition number <= ~100, small angles
 * included (tests/test_gpu_subspace_angles.py).
 * B = NULL: self mode (Bb must equal Ba): the pairs i < j are computed and mirrored, the diagonal is exactly 0.
 * Degenerate basis: a zero (or non-finite) row, or a Cholesky pivot (the diagonal entry before its square root) of the row-normalised block
 * below 1e-10 -- a basis condition number beyond ~1e5.  Every entry of that basis's row / column of theta and dist is NaN (its self-mode diagonal
 * too); no other entry is affected.
 * Reproducibility and batch invariance: no atomics, every sum in a fixed order; theta of a pair is a function of the 2k rows of that pair and of
 * N only -- not of Ba, Bb or the pair's position -- so a pair's result is bitwise the same in a call of its own, in a larger call, and in self
 * mode (i < j) over the concatenation.
 * Limits: 1 <= k <= 128, k <= N, 1 <= Ba, Bb <= 65535.  scratch: 256-byte aligned device memory of scratch_bytes >=
 * dpb_subspace_angles_scratch_bytes(Ba, Bb, k, N) (the fp64 cross-Gram of Ba k x Bb k entries, the whitening matrices, 1024 x 2 k^2 doubles of
 * workgroup scratch); the size is checked.  theta and dist must not alias A, B or scratch.  No device allocation, no host synchronisation.
 * Errors via dpb_last_error. */
int dpb_cross_gram(const float* X, const float* Y /*or NULL: Y = X*/, double* G, int Ra, int Rb, int64_t N, void* hip_stream);
size_t dpb_subspace_angles_scratch_bytes(int Ba, int Bb, int k, int64_t N);   /* 0 when invalid */
int dpb_subspace_angles(const float* A, const float* B /*or NULL: self mode*/, int Ba, int Bb, int k, int64_t N, float* theta, float* dist,
                        void* scratch, size_t scratch_bytes, void* hip_stream);

/* ---- parallel transport of directions between tangent spaces (additive to ABI version 1; engine-independent) ---------------------------
 * The direction arithmetic of run_edit_parallel_transport (src/modules/edit.py:892-909): the source sample's h-space direction u_src[pc] is
 * expressed in a target's h-space basis and carried to x-space through that target's own pairing of u and vT rows,
 *   c[d][p][q] = <uhat_dst[d][q], uhat_src[pcs[p]]>,   w[d][p] = sum_q c[d][p][q] vhat_dst[d][q],   vk[d][p] = w[d][p] / ||w[d][p]||_2,
 * where uhat / vhat are the rows scaled to unit length (the rows need NOT come normalised: u is J V_prev).
 * Inputs, device fp32 row stacks: u_src [k][N_h]; u_dst [D][k][N_h]; vT_dst [D][k][N_x]; pcs: a HOST list of P entries in [0, k), in any order
 * (it travels as a kernel argument).  Outputs, device fp32: vk [D][P][N_x] (unit norm), coef [D][P][k] = c, coef_norm [D][P] = ||c||_2 -- the share of
 * the source direction that the target's h-tangent space holds; it is the cosine of the angle between the direction and that space ONLY when the
 * rows of uhat_dst[d] are orthonormal (for a skewed basis it can exceed 1).
 * Method: the overlaps u_dst u_src^T through dpb_cross_gram (exact products, fp64 accumulation); the row sums of squares of u_src, u_dst and vT_dst
 * in fp64 by a fixed-order reduction; c in fp64, rounded once for coef, and divided by ||vT_dst[d][q]|| in fp64 and rounded once for the streaming
 * kernel; that kernel reads vT_dst once and accumulates w in fp32 with one fma per term in the order q = 0 .. k-1 (so |w - exact| obeys the
 * k-term dot-product bound); ||w||^2 in fp64 from per-workgroup partial sums of the w written, added in a fixed order; one in-place scaling.
 * Degenerate rule: a zero or non-finite source row pcs[p] makes coef, coef_norm and vk of every (d, p) NaN; a zero or non-finite row of u_dst[d] or
 * vT_dst[d], or c[d][p] = 0 exactly, makes them NaN for that (d, p) (w = 0 with c != 0 leaves vk[d][p] NaN alone).  No other entry is affected.
 * Reproducibility and batch invariance: no atomics, every sum one fixed chain that depends on k, N_h and N_x only; the results of target d are
 * bitwise a function of that target's rows, u_src, pcs and the sizes -- the same in a call of its own and inside any stack, whatever the alignment.
 * Limits: 1 <= k <= 128, 1 <= P <= k, 1 <= D <= 65535, N_h, N_x >= 1 (16-byte accesses when the length is a multiple of 4 and the pointers are 16-byte
 * aligned), 64-bit offsets.  scratch: 256-byte aligned device memory of scratch_bytes >= dpb_transport_scratch_bytes(D, P, k, N_h, N_x); the size is
 * checked.  Outputs must not alias inputs or scratch.  No device allocation, no host synchronisation.  Errors via dpb_last_error. */
size_t dpb_transport_scratch_bytes(int D, int P, int k, int64_t N_h, int64_t N_x);   /* 0 when invalid */
int dpb_transport_directions(const float* u_src, const float* u_dst, const float* vT_dst, const int32_t* pcs /*host*/, int P, int D, int k,
                             int64_t N_h, int64_t N_x, float* vk, float* coef, float* coef_norm, void* scratch, size_t scratch_bytes,
                             void* hip_stream);

/* ---- Frechet (Karcher) mean of subspaces on the Grassmannian (additive to ABI version 1; engine-independent) ----------------------------
 * The global basis of run_edit_global_frechet_mean_zt (src/modules/edit.py:951-1246; the reference calls a compute_frechet_basis it never defines
 * and hands the problem to pymanopt): the minimiser Y of (1 / 2B) sum_i ||theta(Y, span X_i)||_2^2 over k-dimensional subspaces, by the Riemannian
 * fixed-step iteration  Y <- Exp_Y(step * (1/B) sum_i Log_Y(X_i)).  X [B][k][N] fp32, one basis per k rows; the rows need NOT be orthonormal, only
 * independent.  R = B k.  There are still no public exponential / logarithm maps: they exist only inside this iteration, on coefficients.
 *
 * Method.  Every iterate lies in the span of the R given rows, so the iteration runs on coefficients: with Q_i = W_i X_i the whitened bases (W_i as
 * in dpb_subspace_angles), Y = C Q, and all it needs is the whitened Gram Ghat = Q Q^T [R][R] fp64, formed once from dpb_cross_gram (exact products).
 * Per step, all fp64: M = C Ghat (block i is Y Q_i^T; one pass over Ghat on the fp64 matrix cores); per basis the eigen-decomposition
 * I - M_i M_i^T = V sin^2(theta) V^T (two-sided Jacobi in LDS), theta = asin(sqrt(l)) for l <= 1/2, else acos(c) with c^2 = ||(V^T M_i)_t||^2 (a sum of
 * squares keeps the relative accuracy of a small cosine, which 1 - l has lost and theta / (sin cos) divides by), and the log map
 * F_i (M_i Q_i - M_i M_i^T Y) with F_i = V theta / (sin cos) V^T; the mean tangent's coefficients C_T; T T^T = (C_T Ghat) C_T^T = P Sigma^2 P^T (the second
 * pass over Ghat, Jacobi); the gradient norm g = ||Sigma||_2 = ||T||_F; C <- P cos(step Sigma) P^T C + P sin(step Sigma) / Sigma P^T C_T, re-orthonormalised
 * by the Cholesky factor of its own Gram.  The cost (1/2) mean_i sum theta^2 of the iterate a step starts from and g are appended to a device history.
 *
 * dpb_frechet_init: forms Ghat and sets C to the identity in block `init` (Y = span X_init); clears the status.
 * dpb_frechet_iterate: n_iter steps.  A step that finds g < tol sets status.done = 1 and does not move Y; a basis whose largest angle to the iterate
 *   exceeds pi/2 - 1e-6 is outside the log map's domain: status.done = 2, status.domain = its index; a full history (max_iter steps): done = 3.  Once
 *   done, the remaining steps of this call and of later calls are no-ops (every kernel reads the flag and returns), so a call never waits for the host.
 * dpb_frechet_finish: the canonical basis of the mean -- C rotated by the eigenvectors of (1/B) sum_i M_i M_i^T, descending; weight [k] fp32 holds the
 *   eigenvalues, the mean cos^2 with which the local spaces hold that direction (row 0: the direction they share most; row signs are whatever the
 *   solve returns, deterministically) -- then Y [k][N] fp32 = (C blockdiag(W)) X in one pass over X (fp32 rows widened on load, summed over the rows in
 *   index order on the fp64 matrix cores, rounded once), theta [B][k] fp32: the principal angles of the mean to every member, descending, and info
 *   [8 + 2 max_iter + 1 + B] fp64: {steps taken, last g, status.done, status.domain, cost entries (steps + 1), re-orthonormalisation failed, 0, 0},
 *   cost [max_iter + 1] (the start included, the final iterate last), g [max_iter] (one per step, one more when done = 1), degenerate flag per basis [B].
 *   finish does not change the state: iterating may go on after it.
 * Status block: the first 32 bytes of scratch are {int32 done, int32 domain, int32 steps, int32 reorth_failed, double g, double cost}; a caller that
 *   iterates in chunks reads them between calls (its only synchronisation).
 * Degenerate basis (the rule of dpb_subspace_angles: a zero or non-finite row, a Cholesky pivot below 1e-10): its flag is set, its blocks of Ghat
 *   are NaN, and NaN spreads to Y, weight, theta and the histories.
 * Reproducibility: no atomics, every sum one fixed chain (the sums over rows are cut at bounds that depend on R only, the sums over bases run in
 *   index order): the result is bitwise the same run to run, and iterate(a) followed by iterate(b) is bitwise iterate(a + b).
 * Limits: 1 <= k <= 64 (three k x k fp64 matrices of the log map live in LDS), k <= N, 1 <= B <= 65535, B k <= 2^20, 0 <= max_iter <= 2^24; 8 R^2
 * bytes of Ghat must fit the scratch.  All three calls take the same B, k, N, max_iter and the same scratch: 256-byte aligned device memory of
 * scratch_bytes >= dpb_frechet_scratch_bytes(B, k, N, max_iter) (checked).  Outputs must not alias X or scratch.  No device allocation, no host
 * synchronisation.  Errors via dpb_last_error. */
size_t dpb_frechet_scratch_bytes(int B, int k, int64_t N, int max_iter);   /* 0 when invalid */
int dpb_frechet_init(const float* X, int B, int k, int64_t N, int init, int max_iter, void* scratch, size_t scratch_bytes, void* hip_stream);
int dpb_frechet_iterate(int n_iter, double step, double tol, int B, int k, int64_t N, int max_iter, void* scratch, size_t scratch_bytes,
                        void* hip_stream);
int dpb_frechet_finish(const float* X, float* Y, float* weight, float* theta, double* info, int B, int k, int64_t N, int max_iter, void* scratch,
                       size_t scratch_bytes, void* hip_stream);

/* dpb_frechet_start (additive): the iteration restarted at a caller's point, after dpb_frechet_init.  Ct [R][k] fp64 on the device: the point's
 * coefficients on the whitened rows, transposed as the state keeps them (Y = C Q; any full-rank C).  It overwrites C in the state, whitens it by the
 * step's own re-orthonormalisation (the Cholesky factor of C Ghat C^T) and clears the status and the histories' count; Ghat is not formed again.
 * dpb_frechet_ghat: the device address of Ghat [R][R] inside a Frechet scratch block (host arithmetic only; NULL with the error set when the
 * arguments are no Frechet problem) -- what dpb_flag_mean_* take as a caller's Ghat. */
const double* dpb_frechet_ghat(int B, int k, int64_t N, int max_iter, const void* scratch);
int dpb_frechet_start(const double* Ct, int B, int k, int64_t N, int max_iter, void* scratch, size_t scratch_bytes, void* hip_stream);

/* ---- Principal geodesic analysis of subspaces (additive to ABI version 1; engine-independent) ----------------------------------------------
 * How the members of a set of local bases vary around a base point Y: PCA of their log maps L_i = Log_Y(span X_i) under <A, B> = tr(A B^T)
 * (geometry.grassmann_pga, the analysis of run_tangent_space_pga).  The calls work on a Frechet scratch block whose point is Y, after
 * dpb_frechet_finish (init alone: a member; init + start: a caller's coefficients; init + iterate: the Karcher mean); nothing of length N is touched
 * before dpb_pga_combine.  `members` is B, or B - 1 when the last basis of the block is a base point stacked by the caller: it is then part of the
 * Gram and of no statistic.  J: the most weight rows one dpb_pga_combine takes (modes + slopes + intercept), 1 <= J <= 80; the same (B, members, k,
 * N, J) and the same pga scratch go to all three calls, in this order.
 *
 * Method.  With Q_i the whitened members, M_i = Y Q_i^T, I - M_i M_i^T = V sin^2(theta) V^T and F_i = V theta / (sin cos) V^T (the log map of
 * dpb_frechet_iterate, the same cosine rule above pi/4), E_i = F_i M_i and K_i = F_i M_i M_i^T: L_i = E_i Q_i - K_i Y, and since Y Y^T = I and
 * Q_a Y^T = M_a^T the inner product closes in k x k algebra, T_ab = tr(E_a Ghat_ab E_b^T) - tr(K_a K_b), T_aa = sum_j theta_aj^2: one pass over Ghat,
 * a workgroup per pair a < b, mirrored (exactly symmetric).  Off the diagonal the two traces are of size k and their difference of size theta^2: an
 * absolute error near k 2^-50, negligible for angles above 1e-4 rad.
 *   dpb_pga_tangent_gram: T [members][members] fp64, theta [members][k] fp32 (descending), state [members] int32: 0 valid, 1 degenerate (the flag of
 *     the whitening), 2 the largest angle to Y exceeds pi/2 - 1e-6 (outside the log map's domain), 4 otherwise not finite.
 *   NaN rule: an invalid member has NaN in its whole row and column of T, the diagonal included, and nowhere else; the rows of a degenerate member are
 *     left out of M = C Ghat, so the other members' entries do not see it.  (dpb_frechet_finish itself returns NaN for Y when a member is degenerate.)
 *   dpb_pga_eig: the members whose diagonal entry is a number are the valid ones, nv of them.  Tc = H T H over them (center != 0; H = I - 1 1^T / nv) or
 *     T, the rows and columns of the others zero.  Tc u = mu u by the round-robin Jacobi in one workgroup while members <= 128 (the matrix in LDS,
 *     160 KiB), above that -- or when dpb_debug_set("pga_route", 2) forces it -- by the flag-mean solver (block subspace iteration with a Rayleigh-Ritz
 *     step, 200 iterations at most, to a residual of 1e-13) on Tc as a Gram of one-row bases.  M <= min(64, members, J) modes in descending order.  Mode
 *     m = sum_i Wt[m][i] L_i, Wt[m] = H u_m / sqrt(mu_m): unit Frobenius norm; sign: the largest-magnitude score is positive; magnitudes within 1e-9 relative of it tie, and the lowest member wins.
 *     An eigenvalue that is not above 1e-13 of the largest, or not above members k 2^-46 (the rounding floor of T), carries no mode: zero weights,
 *     variance and scores.
 *     out fp64 [72 + members M + members]: [0] nv, [1] total variance tr(Tc) / nv, [2] ||mean tangent||_F = sqrt(1^T T 1) / nv, [3] the route (1 Jacobi,
 *     2 subspace), [4] / [5] the subspace solver's iterations and status, [8 .. 8 + M) variance mu_m / nv, then scores [members][M] = sqrt(mu_m) u_mi
 *     (NaN rows for invalid members), then residual [members], residual_i^2 = Tc_ii - sum_m scores_im^2 clamped at 0.
 *   dpb_pga_combine: out fp32 [rows][k][N] = the tangents sum_i Wt[j][i] L_i for `rows` <= J weight rows Wt [rows][members] fp64 on the device (modes
 *     from dpb_pga_eig, or any others: regression slopes, the intercept), invalid members left out.  Coefficients Zq = (blocks w_i E_i) - (sum_i w_i K_i) C
 *     on the whitened rows in fp64, rotated by the rotation dpb_frechet_finish applied to Y -- row j of every output is the image of row j of that Y,
 *     the convention of dpb_grassmann_pair mode 1 / dpb_grassmann_exp -- and composed with the whitenings; then all rows k outputs go through the
 *     coefficient stream of dpb_frechet_finish, 64 output rows per pass over X, summed over the rows of X in index order in fp64, rounded once.
 * Limits: those of dpb_frechet_* (k <= 64, k <= N, B <= 65535, B k <= 2^20).  Scratch: 256-byte aligned, >= dpb_pga_scratch_bytes (checked; 0 when the
 * arguments are invalid).  No atomics, every sum a fixed chain: bitwise reproducible.  No host synchronisation in any call. */
size_t dpb_pga_scratch_bytes(int B, int members, int k, int64_t N, int J);
int dpb_pga_tangent_gram(int B, int members, int k, int64_t N, int max_iter, int J, void* frechet_scratch, size_t frechet_bytes, double* T, float* theta,
                         int32_t* state, void* scratch, size_t scratch_bytes, void* hip_stream);
int dpb_pga_eig(const double* T, int B, int members, int k, int64_t N, int J, int M, int center, double* Wt, double* out, void* scratch, size_t scratch_bytes,
                void* hip_stream);
int dpb_pga_combine(const float* X, const double* Wt, int rows, float* out, int B, int members, int k, int64_t N, int max_iter, int J, void* frechet_scratch,
                    size_t frechet_bytes, void* scratch, size_t scratch_bytes, void* hip_stream);

/* ---- Flag (extrinsic, chordal) mean of subspaces (additive to ABI version 1; engine-independent) -----------------------------------------
 * The global basis of run_edit_global_flag_mean_zt (Draper et al. 2014; Marrinan et al., CVPR 2014): the top-r eigenvectors of the mean projector
 * P = (1/B) sum_i Q_i^T Q_i over the orthonormalised bases Q_i = W_i X_i.  Closed form, no cut locus, defined for every rank r, nested (rows 0..j-1
 * are the rank-j mean); eigenvalue j in [0, 1] is the mean cos^2 with which the members hold row j.  X [B][k][N] fp32 as for dpb_frechet_*; R = B k.
 *
 * Method (csrc/flagmean.hip).  Every row lies in the span of the R given rows, Y = C Q, and P Q^T c = (1/B) Q^T Ghat c with Ghat the whitened Gram of
 * dpb_frechet_init (the same code forms it): the rows of C are eigenvectors of Ghat scaled by lambda^-1/2, so C Ghat C^T = I.  Block subspace
 * iteration on m = min(64, R, 16 ceil((r + 8) / 16)) columns Z [R][m], orthonormal, started at a fixed function of (seed, R, m) (the identity when
 * m = R: one step is then exact); per iteration, all fp64: W = Ghat Z (one pass over Ghat on the fp64 matrix cores, a workgroup per 32 rows);
 * T = Z^T W = S Lambda S^T (two-sided Jacobi in LDS), descending; res = max_{j<r} ||(W S)_j - lambda_j (Z S)_j||_2 / lambda_0; Z <- orth(W S) through
 * the eigen-decomposition of the Gram of W S, twice (W S V D^-1/2, then the symmetric Z1 (Z1^T Z1)^-1/2), directions below 1e-13 of the largest D
 * dropped (Ghat is rank deficient when R > N or members share directions exactly).
 * dpb_flag_mean_init: forms Ghat from X -- or takes the caller's Ghat (X = NULL; dpb_frechet_ghat) -- and the orthonormal start block.
 * dpb_flag_mean_iterate: n_iter iterations.  An iteration that finds res <= tol sets status.done = 1 and does not move the block; a NaN (a degenerate
 *   basis) sets done = 2; max_iter iterations taken: done = 3.  Once done the remaining launches of this and later calls are no-ops.
 * dpb_flag_mean_finish: one more Rayleigh-Ritz step on the block as it stands, taken in the ambient space (the pencil (W^T W, Z^T W): the mean
 *   projector against the Gram of the rows Z^T Q) -- the rows returned are orthonormal and the values returned are their Rayleigh quotients, converged
 *   or not; at convergence they are the eigenpairs.  Y [r][N] fp32 (orthonormal rows, descending eigenvalue; with X: one pass over X, fr_stream_kernel's method), weight [r]
 *   fp32 = lambda_j / B, theta [B][min(r,k)] fp32 (principal angles of span Y to every member, descending; Jacobi on the smaller Gram shape of
 *   M_i = (C Ghat)_i, large angles from the cosine), Ct [R][r] fp64 (C transposed), info [72 + B] fp64: {iterations, status.done, last residual, m, 0,
 *   0, 0, 0}, the m Ritz values (B times the mean cos^2) descending in 64 slots (the oversampled ones included), a degenerate flag per basis.  Sign: each row of C has
 *   its entry of largest magnitude (the lowest index on a tie) positive.  With a caller's Ghat, X = Y = NULL: Y is not formed.  A row beyond the rank of
 *   the stacked rows is zero, with weight 0.  finish leaves the block where it is.
 * Status block: the first 32 bytes of scratch are {int32 done, int32 iterations, int32 0, int32 0, double res, double lambda_0}.
 * Degenerate basis: the rule of dpb_subspace_angles; its blocks of Ghat are NaN, its flag is set, and NaN spreads to every output.
 * Reproducibility: no atomics, every sum one fixed chain whose cut points depend on R and m only: bitwise the same run to run.
 * Limits: 1 <= k <= 64, k <= N, 1 <= B <= 65535, B k <= 2^20, 1 <= r <= min(64, R, N), 0 <= max_iter <= 2^24.  Every call takes the same arguments
 * and the same scratch: 256-byte aligned, dpb_flag_mean_scratch_bytes(B, k, N, r, max_iter) bytes (8 R^2 of them Ghat) -- with a caller's Ghat
 * (32-byte aligned) dpb_flag_mean_solver_bytes(B, k, r, max_iter).  No device allocation, no host synchronisation.  Errors via dpb_last_error. */
size_t dpb_flag_mean_scratch_bytes(int B, int k, int64_t N, int r, int max_iter);   /* 0 when invalid */
size_t dpb_flag_mean_solver_bytes(int B, int k, int r, int max_iter);               /* 0 when invalid */
int dpb_flag_mean_init(const float* X, const double* Ghat, int B, int k, int64_t N, int r, uint64_t seed, int max_iter, void* scratch,
                       size_t scratch_bytes, void* hip_stream);
int dpb_flag_mean_iterate(int n_iter, double tol, const double* Ghat, int B, int k, int64_t N, int r, int max_iter, void* scratch,
                          size_t scratch_bytes, void* hip_stream);
int dpb_flag_mean_finish(const float* X, const double* Ghat, float* Y, float* weight, float* theta, double* Ct, double* info, int B, int k, int64_t N,
                         int r, int max_iter, void* scratch, size_t scratch_bytes, void* hip_stream);

/* ---- Weighted flag mean and flag median (FlagIRLS) of subspaces (additive to ABI version 1; engine-independent) --------------------------
 * Weighted flag mean: the top-r eigenvectors of P_w = sum_i w_i Q_i^T Q_i / sum_i w_i.  Flag median (Mankovich, King, Peterson, Kirby, CVPR 2022): the
 * rank-r subspace minimising sum_i p_i d_i, d_i = sqrt(r - a_i) the chordal distance (not its square), a_i = ||Q_i Y^T||_F^2, 1 <= r <= k, by iteratively
 * reweighted flag means with w_i = p_i / max(d_i, eps); p the caller's weights (uniform when NULL).  A weighted mean is this family with zero rounds.
 *
 * Method (csrc/flagmean.hip).  what = w B / sum w (mean 1, the sum in index order) and D = diag(sqrt(what_i) (x) 1_k): the rows D Q have the Gram
 * D Ghat D, and dpb_flag_mean_*'s solver runs on W = D Ghat D Z -- the same one pass over Ghat with the same cut points and wave-order sum, the scale
 * applied to the Z operand before its MFMAs and to the output row as it is stored (a table of R square roots read through L2; no scaled copy of Ghat):
 * uniform weights give dpb_flag_mean_*'s bits.  Y = C Q with C^T = D Z Sc, C Ghat C^T = I.  M^T = Ghat C^T is a second, UNWEIGHTED pass over Ghat: a
 * member of weight 0 is excluded from the mean and still gets its affinity a_i = ||M[i-rows]||_F^2, distance and angles.
 * dpb_flag_median_init: dpb_flag_mean_init's work (Ghat from X, or the caller's; the start block) and the table from member_weight [B] fp64 on the
 *   DEVICE (NULL: uniform).  A negative or non-finite weight or a zero sum makes the table NaN: the solve then ends with status 2, it does not fault.
 * dpb_flag_median_iterate: dpb_flag_mean_iterate on the weighted product (the inner solve), the status copied to the head.
 * dpb_flag_median_round (r <= k): the Rayleigh-Ritz step of finish under the weighted projector, M, a_i, d_i = sqrt(max(r - a_i, 0)), the smoothed
 *   objective J = sum_i p_i phi(d_i), phi(d) = d for d >= eps and d^2 / (2 eps) + eps / 2 below (what IRLS with the clamped weight descends), in index
 *   order.  From the second round on, J_prev - J <= tol J_prev sets head.converged and moves nothing; otherwise, with update != 0, the new table
 *   what_i = w_i B / sum w and the inner status cleared -- the block Z stays, so the next inner solve is warm-started.  update = 0: J only.
 * dpb_flag_median_finish: dpb_flag_mean_finish's outputs under the table as it stands -- Y [r][N] fp32 (one pass over X), weight [r] fp32 (the Rayleigh
 *   quotients of the WEIGHTED mean projector, in [0, 1]), theta [B][min(r,k)], Ct [R][r], info [72 + B] -- and member [3][B] fp64: affinity, distance,
 *   member weight (what of the last round; the given ones, scaled to mean 1, for a weighted mean).
 * Head: the first 64 bytes of scratch are {int32 round (objective evaluations), int32 done, int32 inner iterations (of the current inner solve),
 *   int32 degenerate members, int32 converged, int32 0, double J, double previous J, double inner residual, 0, 0}: the caller's one read per round.
 * Degenerate basis, reproducibility (fp64, no atomics, every sum one fixed chain), limits and the scratch contract: dpb_flag_mean_*'s, with
 *   dpb_flag_median_scratch_bytes / _solver_bytes.  No device allocation, no host synchronisation.  Errors via dpb_last_error. */
size_t dpb_flag_median_scratch_bytes(int B, int k, int64_t N, int r, int max_iter);   /* 0 when invalid */
size_t dpb_flag_median_solver_bytes(int B, int k, int r, int max_iter);               /* 0 when invalid */
int dpb_flag_median_init(const float* X, const double* Ghat, const double* member_weight /*device [B] or NULL*/, int B, int k, int64_t N, int r,
                         uint64_t seed, int max_iter, void* scratch, size_t scratch_bytes, void* hip_stream);
int dpb_flag_median_iterate(int n_iter, double tol, const double* Ghat, int B, int k, int64_t N, int r, int max_iter, void* scratch,
                            size_t scratch_bytes, void* hip_stream);
int dpb_flag_median_round(double eps, double tol, int update, const double* Ghat, int B, int k, int64_t N, int r, int max_iter, void* scratch,
                          size_t scratch_bytes, void* hip_stream);
int dpb_flag_median_finish(const float* X, const double* Ghat, float* Y, float* weight, float* theta, double* Ct, double* member /*[3][B]*/, double* info,
                           int B, int k, int64_t N, int r, int max_iter, void* scratch, size_t scratch_bytes, void* hip_stream);

/* ---- Chordal affinity of subspaces of unequal rank, and flag k-means (additive to ABI version 1; engine-independent) ---------------------
 * a(A, Y) = sum_j cos^2 theta_j(A, Y) = ||Q_Y Q_A^T||_F^2 in [0, min(r, k)] between a k-dimensional and an r-dimensional subspace of R^N (csrc/flagkmeans.hip).
 *
 * dpb_flag_affinity: A [B][k][N], Y [C][r][N] fp32, rows independent but not necessarily orthonormal; aff [B][C] fp64 on the device,
 *   aff[i][c] = ||W_i (A_i Y_c^T) W'_c^T||_F^2 with W, W' the whitenings of dpb_subspace_angles of each basis's own Gram block: the exact cross-Gram of
 *   dpb_cross_gram, then one workgroup per pair, every element a sequential fp64 sum and the squares added in a fixed order.  Entry (i, c) is bitwise a
 *   function of A_i, Y_c and N alone: the same alone and in any stack.  A degenerate A_i (the rule of dpb_subspace_angles) gives NaN in its row, a
 *   degenerate Y_c in its column.  Limits: 1 <= k, r <= 64, max(k, r) <= N, 1 <= B, C <= 65535.  scratch: 256-byte aligned,
 *   dpb_flag_affinity_scratch_bytes(B, k, C, r, N) bytes (8 B k C r of them the cross-Gram).
 *
 * dpb_flag_kmeans_*: Lloyd's algorithm with rank-r flag means (dpb_flag_mean_*) as centres and r - a as the distance, on coefficients against the
 *   whitened Gram Ghat [R][R] of all R = B k rows; X [B][k][N] fp32 as for dpb_flag_mean_*, 1 <= C <= B clusters, 1 <= r <= k.  The rank-r flag mean of a
 *   cluster maximises the summed affinity of its members, so neither refitting the centres nor moving a member to the centre it holds best can raise
 *   J = sum_i (r - a[i][label_i]).  The CALLER owns the rounds and runs the flag-mean solver per cluster (geometry.flag_kmeans is the loop):
 *   init: Ghat (dpb_frechet_init's code), the seeds and the start labels.  seeds: a HOST list; n_seeds = C gives them all (distinct members), n_seeds = 1
 *     gives seed 0 and each further seed is the member whose smallest D^2(i, s) = k - ||Ghat_is||_F^2 to the seeds so far is largest, the lowest index
 *     on a tie, picked on the device.  Every member takes the nearest seed by D^2, the lowest cluster on a tie; a seed takes its own cluster.
 *   gather: Gc [n_c k][n_c k] = Ghat[I_c][I_c], the members of cluster c ascending, contiguous (32-byte aligned): what dpb_flag_mean_init / _iterate /
 *     _finish take as a caller's Ghat with B = n_c.  n_c must be the cluster's size as the block states it (otherwise nothing is written).
 *   set_centre: files Ct_c [n_c k][r] of dpb_flag_mean_finish (Y_c = Ct_c^T Q[I_c], Ct_c^T Gc Ct_c = I) under its members' rows of Z [R][r].
 *   assign: S[:, c-block] = sum_{j in c} Ghat[:, j-block] Z[j-rows] = Q Y_c^T for every cluster in ONE pass over Ghat on the fp64 matrix cores (a
 *     workgroup per 32 rows and cluster; column block j meets the coefficients of j's own cluster only: 2 R^2 r flops), a[i][c] = ||S[i-rows, c-block]||_F^2,
 *     J, and with apply != 0 the moves: member i goes to argmax_c a[i][c] (lowest c on a tie) if that exceeds a[i][label_i] by more than 1e-12 r; a
 *     cluster none of whose members wants to stay keeps the one of largest affinity to it (lowest index on a tie), so a cluster never empties; then
 *     the new labels, sizes, member lists and the clusters whose member set changed.  apply = 0: a and J of the labels as they stand.
 *   finish: Y [C][r][N] fp32 from the coefficients on the rows as given (Z blockdiag(W), zero outside a centre's members) by the streaming pass of
 *     dpb_flag_mean_finish: one pass over X when C r <= 64, otherwise one per cluster.
 * Host part: the first dpb_flag_kmeans_host_bytes(...) bytes of scratch are {int32 moved, int32 kept, int32 degenerate members, int32 0, double J,
 *   double 0}, then int32 sizes [C], changed [C], seeds [C], labels [B] (-1: degenerate) and degenerate flags [B]: the caller's one read per round.
 *   dpb_flag_kmeans_affinity: the device address of a [B][C] fp64 inside the block (host arithmetic only; NULL with the error set when invalid).
 * Degenerate member (the rule of dpb_subspace_angles): its flag is set, its label is -1, it joins no cluster and no sum, its row of a is NaN.
 * Reproducibility: fp64, no atomics, every sum one fixed chain; the reduction range of the assignment pass is cut among the waves of a workgroup at
 *   bounds that depend on the member list only and the partial tiles are added in wave order: bitwise the same run to run.
 * Limits: 1 <= k <= 64, k <= N, 1 <= B <= 65535, B k <= 2^20, 1 <= C <= B, 1 <= r <= k.  Every call takes the same B, k, N, C, r and the same scratch:
 *   256-byte aligned, dpb_flag_kmeans_scratch_bytes(B, k, N, C, r) bytes (8 R^2 of them Ghat, 8 R C r the products S).  init synchronises the stream
 *   once (the seeds' copy); nothing else synchronises or allocates.  Errors via dpb_last_error. */
size_t dpb_flag_affinity_scratch_bytes(int B, int k, int C, int r, int64_t N);   /* 0 when invalid */
int dpb_flag_affinity(const float* A, const float* Y, int B, int k, int C, int r, int64_t N, double* aff /*[B][C]*/, void* scratch, size_t scratch_bytes,
                      void* hip_stream);
size_t dpb_flag_kmeans_scratch_bytes(int B, int k, int64_t N, int C, int r);     /* 0 when invalid */
size_t dpb_flag_kmeans_host_bytes(int B, int k, int64_t N, int C, int r);        /* 0 when invalid */
const double* dpb_flag_kmeans_affinity(int B, int k, int64_t N, int C, int r, const void* scratch);
int dpb_flag_kmeans_init(const float* X, int B, int k, int64_t N, int C, int r, const int32_t* seeds /*host [n_seeds]*/, int n_seeds, void* scratch,
                         size_t scratch_bytes, void* hip_stream);
int dpb_flag_kmeans_gather(int c, int n_c, double* Gc /*[n_c k][n_c k]*/, int B, int k, int64_t N, int C, int r, void* scratch, size_t scratch_bytes,
                           void* hip_stream);
int dpb_flag_kmeans_set_centre(int c, int n_c, const double* Ct /*[n_c k][r]*/, int B, int k, int64_t N, int C, int r, void* scratch,
                               size_t scratch_bytes, void* hip_stream);
int dpb_flag_kmeans_assign(int apply, int B, int k, int64_t N, int C, int r, void* scratch, size_t scratch_bytes, void* hip_stream);
int dpb_flag_kmeans_finish(const float* X, float* Y /*[C][r][N]*/, int B, int k, int64_t N, int C, int r, void* scratch, size_t scratch_bytes,
                           void* hip_stream);

/* ---- Grassmann geodesics: principal vectors, log and exp maps (additive to ABI version 1; engine-independent) --------------------------
 * Pairs (A_d, B_d), d < D, of bases of k rows in R^N, fp32, rows independent but not necessarily orthonormal (ROWS convention).  a_stride = k N:
 * A [D][k][N]; a_stride = 0: one A [k][N] paired with every B_d.  Everything between input and output is fp64 (csrc/geodesic.hip).
 * Method, per pair, from the exact Grams A A^T, B B^T, A B^T (dpb_cross_gram) and the whitenings Wa, Wb of dpb_subspace_angles:
 *   M = Wa (A B^T) Wb^T;  I - M M^T = V sin^2(theta) V^T (two-sided Jacobi with vectors);  U = V^T M, row i of norm cos(theta_i);  theta from
 *   asin(sqrt(lambda)) for lambda <= 1/2 and from acos ||U_i|| above, DESCENDING with ties by index (the order of dpb_subspace_angles);
 *   principal vectors Pa = (V^T Wa) A, Pb = (diag(1 / cos theta) U Wb) B: orthonormal rows, Pa Pb^T = diag(cos theta), cos theta >= 0; sign: the
 *   entry of largest magnitude of each row of V^T (lowest index on ties) is positive.
 *   Every output row is alpha_i pa_i + beta_i pb_i, formed in fp64 from the two rotated tiles in ONE pass over the 2k rows (fp64 matrix cores, rows
 *   summed in index order) and rounded to fp32 once:
 *     mode 2, geodesic from span A (t = 0) to span B (t = 1), any real t: alpha = sin((1 - t) theta) / sin theta, beta = sin(t theta) / sin theta
 *       (1 - t and t where sin theta = 0);
 *     mode 1, log map: the tangent at span A is the linear map pa_i -> h_i = (theta_i / sin theta_i)(pb_i - cos theta_i pa_i); h_i is orthogonal to
 *       span A, ||h_i|| = theta_i, ||H||_F the geodesic distance.
 *   out0 / out1: mode 0: Pa, Pb, each [D][k][N]; mode 1: Pa, H; mode 2: Y [D][J][k][N] at ts[0 .. J) (a HOST array), out1 NULL.  theta [D][k] fp32.
 * dpb_grassmann_exp: P_d, H_d [k][N] (each [D][k][N]); the tangent at span P is the linear map p_i -> the component of h_i orthogonal to span P (well
 *   defined for a non-orthonormal P; H is arbitrary).  With W the whitening of P, Q = W P, K = (W H) Q^T and Hq = W H - K Q as coefficients on the 2k
 *   given rows: Hq Hq^T = W (H H^T) W^T - K K^T = V sigma^2 V^T (Jacobi), sigma descending, and row i of Y[d][j] is
 *   cos(t_j sigma_i) (V^T Q)_i + (sin(t_j sigma_i) / sigma_i) (V^T Hq)_i (the second coefficient is t_j at sigma_i = 0).  sigma [D][k] fp32.  No
 *   domain limit.  exp of the (P, H) of mode 1 reproduces the geodesic of mode 2 as a subspace.
 * flags [D]: 0 ok; 1 a degenerate basis of the pair (the whitening's rule: a zero or non-finite row, a Cholesky pivot of the row-normalised Gram
 *   below 1e-10); 2 (dpb_grassmann_pair only) the largest principal angle exceeds pi/2 - 1e-6: the geodesic is not unique at the cut locus and
 *   1 / cos theta is unbounded.  A flagged pair has NaN in ALL its outputs; it spoils no other pair.
 * Reproducibility: no atomics, every sum one fixed chain: a pair's result is bitwise the same alone, at any position of any stack, and with A
 *   broadcast (a_stride = 0).
 * Limits: 1 <= k <= 64 (three k x k fp64 matrices and the Jacobi workspace live in LDS), k <= N, 1 <= D <= 65535, 1 <= J <= 64, a_stride in {0, k N}.
 *   scratch: 256-byte aligned device memory of scratch_bytes >= dpb_grassmann_scratch_bytes(D, J, k, N) (checked; J = 2 for modes 0 and 1).  The
 *   accuracy is that of the Gram route: a general mixing of the rows of condition c loses sqrt(eps) c at small angles (row scaling does not: the
 *   whitening removes it first).  Outputs must not alias inputs or scratch.  No device allocation, no host synchronisation.  Errors via dpb_last_error. */
size_t dpb_grassmann_scratch_bytes(int D, int J, int k, int64_t N);          /* 0 when invalid (k outside [1, 64], k > N, ...) */
int dpb_grassmann_pair(const float* A, int64_t a_stride /*0: one A for all D*/, const float* B, int D, int k, int64_t N,
                       int mode /*0 principal vectors, 1 log, 2 geodesic*/, const double* ts /*host [J], mode 2*/, int J,
                       float* out0, float* out1, float* theta /*[D][k]*/, int32_t* flags /*[D]: 0 ok, 1 degenerate, 2 domain*/,
                       void* scratch, size_t scratch_bytes, void* hip_stream);
int dpb_grassmann_exp(const float* P, const float* H, int D, int k, int64_t N, const double* ts /*host [J]*/, int J,
                      float* Y /*[D][J][k][N]*/, float* sigma /*[D][k]*/, int32_t* flags, void* scratch, size_t scratch_bytes, void* hip_stream);

/* ---- the Hungarian-matched mean of directions (additive to ABI version 1; engine-independent) -----------------------------------------
 * The global basis of run_edit_global_hungarian_mean_zt (src/modules/edit.py:1249-1514; the reference calls a compute_hungarian_basis it never
 * defines, with initial_local_basis_idx=0, distance='1/cosine').  Where the Frechet mean averages subspaces, this one averages DIRECTIONS: the k rows
 * of every basis are matched one to one, and sign by sign, to the rows of an anchor, and the matched unit vectors are averaged.  X [B][k][N] fp32,
 * one basis per k rows; rows need not be unit length (xhat: a row divided by its fp64 norm), and nothing here needs them orthogonal.
 *
 * dpb_linear_assignment: the batched solver.  cost [B][k][k] fp64, row-major; col_of_row [B][k] int32 and total [B] fp64 out: the permutation that
 *   minimises sum_i cost[b][i][col_of_row[b][i]], and that sum (added in row order).  One workgroup per problem; the shortest-augmenting-path
 *   (Jonker-Volgenant) method in fp64 with the matrix, the duals, the predecessors and both matchings in LDS; every Dijkstra step relaxes all
 *   unscanned columns at once and takes the (value, index) minimum that breaks ties on the LOWEST column index, so the result is a function of the
 *   matrix alone: problem b is bitwise the same alone and in any batch, run to run.  Among several optimal assignments it returns one; its total is
 *   the optimum.  Costs must be finite: a problem with a NaN or an infinity (or whose path sums overflow) gets col_of_row = -1 and total = NaN, and no
 *   other problem is touched.  Limits: 1 <= k <= 128 (8 k^2 bytes of LDS: 128 KiB at k = 128; a 32 KiB instantiation serves k <= 64),
 *   1 <= B <= 2^20.  scratch: 256-byte aligned device memory of >= dpb_linear_assignment_scratch_bytes(B, k) bytes (checked; the block is reserved:
 *   the solver's state lives in LDS).
 *
 * dpb_matched_mean: ONE sweep.  anchor [k][N] fp32, or NULL for X[init] (0 <= init < B; ignored when anchor is given).  With yhat the anchor's unit
 *   rows: c_b[i][j] = <yhat_i, xhat_{b,j}> from dpb_cross_gram(anchor, X) (exact products) divided by the row norms (the fixed-order fp64 sums of
 *   squares of dpb_row_sumsq), the cost d = 1 / max(|c|, 2^-40) (distance 0, '1/cosine') or 1 - |c| (distance 1, 'cosine'), formed in fp64 while the
 *   solver loads its matrix; perm[b] = the assignment of d (as dpb_linear_assignment), sign[b][i] = -1 if c_b[i][perm[b][i]] < 0, else +1; then
 *   Y[i] = normalise(sum_b sign[b][i] xhat_{b, perm[b][i]}): one pass over X, b in index order, one fp64 fma per term, the norm from per-chunk partial
 *   sums added in chunk order, ONE rounding to fp32.  Row i of Y is the direction matched to anchor row i.
 *   perm, sign [B][k] int32 are read as the previous sweep's assignment and written as the new one (first sweep: fill perm with -1).
 *   info [1 + 2 B] fp64: {the number of (b, i) entries whose perm or sign changed, total cost per basis [B], degenerate flag per basis [B]}.  The caller
 *   owns the sweeps: Y of one call is the anchor of the next, until info[0] == 0 (one host read per sweep) or its cap; with 'cosine' a sweep cannot
 *   decrease sum_b sum_i |<y_i, xhat_{b,perm}>|, with '1/cosine' nothing guarantees termination.
 *   Degenerate basis (the rule of dpb_transport_directions: a zero or non-finite row, in basis b or in the anchor): its flag is 1, its perm -1, its
 *   sign 0, its total NaN, and NaN spreads to Y.
 *   Reproducibility and batch invariance: no atomics, every sum one fixed chain; perm[b], sign[b] and total[b] are a function of the anchor, the rows
 *   of basis b, k and N only -- bitwise the same in a call of its own and inside any stack; Y is bitwise the same run to run.
 *   Limits: 1 <= k <= 128, 1 <= B <= 2^20, B k <= 2^24, N >= 1 (any N; 16-byte accesses when N % 4 == 0 and the pointers are 16-byte aligned,
 *   64-bit offsets throughout).  scratch: 256-byte aligned, >= dpb_matched_mean_scratch_bytes(B, k, N) (checked): the k x B k overlaps, the row
 *   norms, and the fp64 sums [k][N] before they are normalised.  Y must not alias X, anchor or scratch.
 *
 * dpb_row_sumsq: ss[r] = sum_n X[r][n]^2 in fp64, X [rows][N] fp32 -- the fixed-order reduction the transport and the matched mean use (a chain
 *   that depends on N only).
 * No device allocation, no host synchronisation.  Errors via dpb_last_error. */
size_t dpb_linear_assignment_scratch_bytes(int B, int k);   /* 0 when invalid */
int dpb_linear_assignment(const double* cost /*[B][k][k]*/, int B, int k, int32_t* col_of_row /*[B][k]*/, double* total /*[B]*/, void* scratch,
                          size_t scratch_bytes, void* hip_stream);
size_t dpb_matched_mean_scratch_bytes(int B, int k, int64_t N);   /* 0 when invalid */
int dpb_matched_mean(const float* X, int B, int k, int64_t N, const float* anchor /*[k][N] or NULL: X[init]*/, int init, int distance,
                     float* Y /*[k][N]*/, int32_t* perm /*[B][k]*/, int32_t* sign /*[B][k]*/, double* info /*[1 + 2 B]*/, void* scratch,
                     size_t scratch_bytes, void* hip_stream);
int dpb_row_sumsq(const float* X, int64_t rows, int64_t N, double* ss /*[rows]*/, void* hip_stream);

/* n_iters full power iterations with no host synchronisation: V <- orth(J^T J V), U = J V_prev, for all B samples
 * of the last dpb_primal together (independent bases, one shared weight stream; B*k <= max_tangents).
 * V [B][k][N_in] in/out, U [B][k][N_h] out, s [B][k] out, conv [B][2] out (of the last iteration).
 * Non-finite values follow the rule of dpb_orth per sample: a sample whose V or W = J^T J V holds a NaN or an inf (an fp16 tangent that overflowed)
 * comes back with V and s all NaN and conv = (NaN, NaN), and stays so in the following iterations; no other sample's V, U, s or conv changes by a
 * bit; the call returns 0.  A caller that reads conv for a stop rule must treat a non-finite conv as an error, never as converged.
 * Replaces: the loop body utils.py:756-808 (k <= 128), once per sample of the batch. */
int dpb_pullback_iterate(dpb_engine* e, int tap_buf, float* V, float* U, float* s, float* conv, int k, int n_iters);

/* ---- the decoder pullback: passes seeded at an inner activation (additive to ABI version 1) -----------------------------
 * J_dec = d eps / d h of the tap-to-output map, every skip connection held at its primal value (reference: PullBackDDPM.get_h_to_e,
 * src/models/ddpm/diffusion.py:273-345; utils.get_h_to_e, src/utils/utils.py:529-635).  src_buf is the seed (a tap h), dst_buf a buffer
 * downstream of it (the eps buffer).  A buffer carries a tangent / cotangent in these passes iff it is reachable forward from src_buf; the
 * others (skip activations, the time-embedding and text paths, everything upstream of src_buf) are constants.  With src_buf = x_buf the
 * passes are exactly dpb_jvp / dpb_vjp / dpb_pullback_iterate.  Primal state: dpb_primal(..., upto_buf = dst_buf or later) keeps everything
 * these passes read (its stash already covers the whole prefix of the tape); a primal that stops before dst_buf is refused, as are a dst_buf
 * not downstream of src_buf, dpb_forward's missing state and k outside [1, 128]; errors via dpb_last_error.
 * V fp32 NCHW [nt][channels(src)][rows(src)], U fp32 NCHW [nt][channels(dst)][rows(dst)] (valid channels).
 * Replace: torch.func.jacfwd of get_h_to_e (diffusion.py:599-602, utils.py:863-866) and autograd.functional.jacobian (diffusion.py:614-616,
 * utils.py:878-880). */
int dpb_jvp_between(dpb_engine* e, int src_buf, int dst_buf, const float* V, int nt, float* U);
int dpb_vjp_between(dpb_engine* e, int src_buf, int dst_buf, const float* U, int nt, float* W);
/* Device scratch the iteration below needs for k directions per sample, at the engine's max_batch: the fp32 staging of W = J^T J V and one
 * re-orthonormalisation slot per sample, both sized by N = numel(src_buf) -- the caller provides it, so the engine workspace
 * (dpb_engine_workspace_bytes) does not grow for engines that never run the decoder.  0 for an invalid src_buf or k outside [1, 128]. */
size_t dpb_pullback_scratch_bytes(const dpb_engine* e, int src_buf, int k);
/* dpb_pullback_iterate between src_buf and dst_buf: V [B][k][N_src] in/out, U [B][k][N_dst] out (J V_prev of the last iteration), s [B][k],
 * conv [B][2]; no host synchronisation.  scratch: 256-byte aligned device memory of scratch_bytes >= what B = the last primal's batch needs
 * (dpb_pullback_scratch_bytes is enough for any B).  Replaces: the loop body of local_decoder_pullback_xt / _zt (diffusion.py:592-625,
 * utils.py:856-890), k <= 128. */
int dpb_pullback_iterate_between(dpb_engine* e, int src_buf, int dst_buf, float* V, float* U, float* s, float* conv, int k, int n_iters,
                                 void* scratch, size_t scratch_bytes);
/* Forward from a tap (get_h_to_e): the primal to src_buf at `batch` samples of x (the caller repeats x), P(src_buf) overwritten by h
 * (fp32 NCHW [batch][channels(src)][rows(src)]), then on to dst_buf, copied out like dpb_forward (whose state rules it shares: no primal
 * state afterwards).  Replaces: get_h_to_e with input_h.size(0) = batch (utils.py:593-606, diffusion.py:321-325: the skips repeated). */
int dpb_forward_from(dpb_engine* e, const float* x, int batch, float t, const float* ctx, int src_buf, const float* h, int dst_buf, int channels,
                     float* out);
/* The h-space shifted forward (additive to ABI version 1): row b of `out` is dst_buf of the net with the activation at src_buf replaced by
 * h(x_b) + scale[b] * u[dir[b]] and every skip taken from x_b.  u: DEVICE fp32 [nu][channels(src)][rows(src)] (NCHW-flattened, valid channels);
 * dir, scale: HOST arrays of `batch` entries -- they travel as kernel arguments, dir[b] = -1 leaves row b unshifted.  The sum is formed in fp32
 * and rounded once to the engine dtype.  xbatch = batch: x [batch] and ctx [batch] rows, one ordinary forward pass with the shift applied right
 * after the producer of src_buf.  xbatch = 1 < batch (shared prefix): x [1], ctx [1]; the ops up to the producer of src_buf run ONCE at batch 1,
 * the tap is written as `batch` shifted copies, sample 0 of every buffer the rest of the pass still reads (skips, the context's K/V projection;
 * derived from the tape) is broadcast in one launch, and only the ops after the tap run at `batch`.  No device allocation, no host synchronisation
 * beyond dpb_forward's one for the timestep embedding; state rules of dpb_forward (no primal state afterwards); dpb_engine_stats reports what was
 * launched.  Refused (dpb_last_error): batch outside [1, max_batch], xbatch not in {1, batch}, nu < 1, a dir[b] outside [-1, nu), src_buf not an
 * x-dependent activation produced by an op, dst_buf not strictly downstream of src_buf.
 * Replaces: PullBackDDPM.forward(x, t, u, op, block_idx) (src/models/ddpm/diffusion.py:145-200) and forward_dh (src/utils/utils.py:350-436). */
int dpb_forward_shift(dpb_engine* e, const float* x, int xbatch, int batch, float t, const float* ctx, int src_buf, const float* u, int nu,
                      const int32_t* dir, const float* scale, int dst_buf, int channels, float* out);

/* DDIM update (utils.py:301-306 / :1220-1225, eta = 0) and the x-space-guidance axpy (edit.py:490, :501). */
int dpb_ddim_step(const float* x, const float* eps, float* out, float* x0, int64_t n, float alpha_t, float alpha_next,
                  void* hip_stream);
int dpb_lincomb(const float* x, const float* y, const float* z, float* out, int64_t n, float a, float b, float c,
                void* hip_stream);

/* ---- the parallel-h edit chain (additive to ABI version 1) --------------------------------------------------------------------------
 * The --edit_xt parallel-h branch of the global-basis edit jobs (src/modules/edit.py:1202-1229, :1470-1497): the h-space direction c is held fixed and
 * the x-space direction is recomputed at every state, v = -J^T c / ||J^T c|| (PullBackDDPM.inv_jac_xt, src/models/ddpm/diffusion.py:347-377),
 * x <- x + step v, optionally with the SEGA rule v <- where(|v| < sega_sigma std(v), 0, v).  Sign: a chain with sign = +1 moves h AGAINST c,
 * <h - h0, c> / ||c|| ~ -step ||J^T c|| / ||c|| at first order (the reference's convention, kept).
 *
 * dpb_direction_step (engine-independent): W [n][N] fp32 (the adjoint results J^T c), x [n][N], x_out [n][N] (may alias x: every element is read by
 * the thread that overwrites it), vk [n][N] or NULL, step: a HOST array of n entries, stats [n][4] FP64 on the device.  Per row b:
 *   S1 = sum w, S2 = sum w^2 in fp64 (fp32 widened on load; per-workgroup partial sums of slices of 4096 elements, added in slice order; no atomics:
 *   the sums are a function of the row and N only); v_i = fl32(-w_i / sqrt(S2)), formed in fp64 and rounded once; when sega_sigma > 0 and N >= 2,
 *   std = sqrt(max(0, 1 - S1^2 / (N S2)) / (N - 1)) -- torch's unbiased std of the unit-norm row, in the two sums -- and v_i <- 0 where
 *   |v_i| < sega_sigma std, compared in fp64 (N = 1: v is left alone; the reference's std is NaN there and its where keeps the element);
 *   x_out_i = fl32(x_i + step_b v_i), formed in fp64 and rounded once; stats[b] = (S2, std or 0, elements the rule kept (N when it is off), flag).
 *   A row with S2 == 0 or S2 not finite: flag = 1, std = 0, kept = 0, and NaN in exactly that row of vk and x_out; no other row changes by a bit.
 * Two launches per 256 rows (partial sums, apply: every apply workgroup re-adds the row's partials in index order); the kept count is a sum of
 * integers below 2^53 and the one place an (fp64, exact) atomic is used.  A row's results are bitwise the same alone and at any position of a stack,
 * whatever the alignment: rows start at b N floats, and each workgroup takes 16-byte accesses for an aligned row, 4-byte ones otherwise, with the
 * same elements per thread.  scratch: 8-byte aligned device memory of >= dpb_direction_step_scratch_bytes(n, N) bytes.  Refused: a non-finite step[b],
 * a NaN sega_sigma.  No host synchronisation.
 * dpb_shift_stats (engine-independent): h [n][D], h0 [n][D], u [nu][D] fp32 on the device, dir [n] in [0, nu) and sign [n] HOST arrays;
 * out [n][2] FP64 on the device = (<h - h0, c> / ||c||, ||h - h0||^2) with c = sign[b] u[dir[b]], fixed-order fp64 sums, no atomics.
 *
 * dpb_inv_jac_chain: n chains advanced together for `steps` steps, no host work between the steps.  x [n][N_in] fp32 NCHW, t: a HOST array of n
 * timesteps (the rules of dpb_primal_t), ctx [n][L][Dc] or NULL, u [nu][N_h] fp32 NCHW-flattened directions of the tap, dir / sign / step HOST
 * arrays of n entries: chain b follows c_b = sign[b] u[dir[b]] with step[b] per step.  states [steps + 1][n][N_in]: states[0] = x (states may
 * start at x); step j runs dpb_primal_t at states[j] up to the tap, gathers the cotangents c_b on the device, runs the adjoint pass of dpb_vjp with
 * one cotangent per sample, and dpb_direction_step into states[j + 1] (vk [steps][n][N_in] or NULL, stats [steps][n][4]).  shift [steps + 1][n][2]:
 * dpb_shift_stats of the tap activation the primal pass of step j has just produced against the copy kept from step 0 (row 0 is (0, 0)); row
 * `steps` takes one more forward pass to the tap when final_shift != 0, else it is NaN.
 * Host synchronisation: ONE for the call -- the upload of the timestep embeddings in step 0; they stay resident in the engine for the other steps
 * (as the chunks of dpb_local_pca_sample).  No device allocation: scratch is 256-byte aligned device memory of >=
 * dpb_inv_jac_chain_scratch_bytes(e, tap_buf, n) bytes (0 when invalid).  The call leaves no primal state, as dpb_forward.
 * Refused (dpb_last_error): n outside [1, min(max_batch, max_tangents)], steps < 1, nu < 1, a dir[b] outside [0, nu), a non-finite t[b], sign[b] or
 * step[b], a tap that is not an x-dependent activation, a missing ctx, scratch too small or misaligned. */
size_t dpb_direction_step_scratch_bytes(int64_t n, int64_t N);   /* 0 when invalid */
int dpb_direction_step(const float* W, const float* x, float* x_out, float* vk /*or NULL*/, const float* step /*host [n]*/, float sega_sigma,
                       int64_t n, int64_t N, double* stats /*dev [n][4]*/, void* scratch, size_t scratch_bytes, void* hip_stream);
int dpb_shift_stats(const float* h, const float* h0, const float* u, int nu, const int32_t* dir /*host [n]*/, const float* sign /*host [n]*/,
                    int64_t n, int64_t D, double* out /*dev [n][2]*/, void* hip_stream);
size_t dpb_inv_jac_chain_scratch_bytes(const dpb_engine* e, int tap_buf, int n);
int dpb_inv_jac_chain(dpb_engine* e, int tap_buf, const float* x /*dev [n][N_in]*/, int n, const float* t /*host [n]*/,
                      const float* ctx /*dev [n][L][Dc] or NULL*/, const float* u /*dev [nu][N_h]*/, int nu, const int32_t* dir,
                      const float* sign, const float* step /*host [n]*/, int steps, float sega_sigma, int final_shift,
                      float* states /*dev [steps+1][n][N_in]*/, float* vk /*dev [steps][n][N_in] or NULL*/, double* stats /*dev [steps][n][4]*/,
                      double* shift /*dev [steps+1][n][2]*/, void* scratch, size_t scratch_bytes);

/* ---- the least-squares inverse of the Jacobian and the newton-h chain (additive to ABI version 1) ---------------------------------------
 * The reference's inv_jac_xt aims at argmin_v ||perturbed_h - f(xt + v)|| (src/models/ddpm/diffusion.py:369) and takes ONE gradient of that norm:
 * the steepest-descent direction -J^T c / ||J^T c||, which the parallel-h chain above follows.  This section is the minimiser itself: CGLS on
 *   min_d ||J d - c||^2 + mu ||d||^2   from d = 0   (at mu = 0 and enough iterations: the minimum-norm solution J^+ c),
 * with the tangent and adjoint passes of the engine for the products with J and J^T, and a damped Gauss-Newton chain built on it.
 *
 * The solver kernels (engine-independent), R independent rows per call.  Row b carries d_b, p_b [N], r_b [D] fp32 and state[b][8] FP64 on the device =
 * (gamma, gamma0, mu_b, ||r||^2, ||d||^2, flag, ||c||^2, x-steps taken); alpha and beta never leave the device.
 *   dpb_cgls_init    c [R][D], w0 [R][N] (= J^T c, supplied): d = 0, r = c, p = w0, gamma = gamma0 = ||w0||^2, mu_b = mu_abs + mu_rel gamma0 / ||c||^2
 *   dpb_cgls_h_step  q [R][D] (= J p):        alpha = gamma / (||q||^2 + mu_b ||p||^2), d <- fl32(d + alpha p), r <- fl32(r - alpha q)
 *   dpb_cgls_x_step  w [R][N] (= J^T r):      s = w - mu_b d (fp64, not stored), gamma' = ||s||^2, beta = gamma' / gamma, p <- fl32(s + beta p),
 *                                             gamma <- gamma'
 * d, r and p are updated in place.  Every sum is in fp64 over fp32 operands widened on load: per-workgroup sums of slices of 4096 elements, added in
 * slice order by every workgroup that needs the total; no floating-point atomics.  Every new element is formed in fp64 and rounded once.  A row
 * takes 16-byte accesses when it is aligned and 4-byte ones otherwise, with the same elements per thread: a row's bits depend on that row, N and D
 * only -- the same alone, anywhere in a stack and at any alignment.  Three launches per 256 rows and call (slice sums, apply, one thread per row for
 * the scalars).  Each call writes one history row hist[b] = (gamma, ||r||^2, ||d||^2, flag) FP64 on the device.  Flags:
 *   1  gamma <= tol^2 gamma0 (gamma0 = 0 included), set by init and by the x-step: converged.  The row FREEZES: every later step leaves its d, r, p
 *      and state as they are, bit for bit, and reads none of its inputs (in fp32 a row iterated past its floor moves away from the solution again);
 *   2  a zero or non-finite denominator (||q||^2 + mu_b ||p||^2 in the h-step; ||c||^2 = 0 with w0 != 0, or a non-finite mu_b, at init): frozen too;
 *   3  a non-finite input (c or w0; q or p; w): NaN in d, r, p and in the scalars of exactly that row, frozen.
 * scratch: 8-byte aligned device memory of >= dpb_cgls_*_scratch_bytes(R, N, D) bytes (the three sizes are equal: one block serves a whole
 * solve).  Refused (dpb_last_error): a null argument, R < 1, N < 1, D < 1, a negative or non-finite mu_abs /
 * mu_rel / tol, scratch too small, scratch / state / hist not 8-byte aligned.  No host synchronisation.
 *
 * dpb_newton_residual (engine-independent): res[b] = fl32(h0[b] + (frac scale[b]) (sign[b] u[dir[b]]) - h[b]), formed in fp64 and rounded once;
 * h0, h, res [n][D], u [nu][D] fp32 on the device, dir / sign / scale HOST arrays.  dpb_newton_update (engine-independent): x_out[b] =
 * fl32(x[b] + kappa_b d[b]) with kappa_b = min(1, radius / ||d_b||) (radius = 0: no clamp), ||d_b||^2 read from the solver's state;
 * step_stats[b] = (||res||^2, ||d||^2, kappa, flag) FP64 on the device, the first and the last from the state as well.
 *
 * dpb_jac_lstsq: the solve on the primal state dpb_primal / dpb_primal_t left, with dpb_jvp's row convention -- row j belongs to sample
 * j / (nt / batch), so one sample with k right-hand sides and n samples with one each are the same call.  One adjoint pass for w0, dpb_cgls_init, then
 * `iters` rounds of tangent pass, h-step, adjoint pass, x-step; no host work or synchronisation between them.  The passes run for frozen rows too
 * (the batch shape never changes).  c [nt][N_h], delta [nt][N_in], resid [nt][N_h] or NULL (c - J delta, as the recurrence carries it),
 * hist [iters + 1][nt][4]: row 0 from init, row i from round i.  p goes into the tangent pass as it is (||p|| ~ ||J^T c||): on a 16-bit engine a
 * right-hand side large enough to overflow the tangent activations ends as flag 3; the problem is linear, scale c down and delta up.  The primal state stays usable, as after dpb_jvp.  scratch: 256-byte aligned device
 * memory of >= dpb_jac_lstsq_scratch_bytes(e, tap_buf, nt) bytes (0 when invalid).  Refused: what dpb_jvp refuses, iters < 0, and the solver's.
 *
 * dpb_newton_h_chain: n chains advanced together; chain b aims at h0_b + scale[b] c_b, c_b = sign[b] u[dir[b]].  Sign: a chain with sign = +1 moves
 * h ALONG c -- the opposite of dpb_inv_jac_chain, which keeps the reference's sign.  Outer step j of `steps`: dpb_primal_t at states[j] up to the
 * tap and dpb_shift_stats against the h0 kept from step 0 (shift[j]); res = dpb_newton_residual at frac = (j + 1) / steps; the solve of dpb_jac_lstsq
 * on it (hist [steps][iters + 1][n][4]); states[j + 1] = dpb_newton_update (step_stats [steps][n][4]).  shift[steps]: one more forward pass when
 * final_shift != 0, else NaN.  Host synchronisation: ONE for the call, the upload of the timestep embeddings in step 0.  No device allocation:
 * scratch is 256-byte aligned device memory of >= dpb_newton_h_chain_scratch_bytes(e, tap_buf, n) bytes (0 when invalid).  The call leaves no primal
 * state, as dpb_forward.  Refused: what dpb_inv_jac_chain refuses (scale in the place of step), a negative or non-finite radius, and the solver's. */
size_t dpb_cgls_init_scratch_bytes(int64_t R, int64_t N, int64_t D);     /* 0 when invalid */
int dpb_cgls_init(const float* c, const float* w0, float* delta, float* r, float* p, double* state /*dev [R][8]*/, double* hist /*dev [R][4]*/,
                  double mu_abs, double mu_rel, double tol, int64_t R, int64_t N, int64_t D, void* scratch, size_t scratch_bytes, void* hip_stream);
size_t dpb_cgls_h_step_scratch_bytes(int64_t R, int64_t N, int64_t D);
int dpb_cgls_h_step(const float* q, float* delta, float* r, float* p, double* state, double* hist, int64_t R, int64_t N, int64_t D, void* scratch,
                    size_t scratch_bytes, void* hip_stream);
size_t dpb_cgls_x_step_scratch_bytes(int64_t R, int64_t N, int64_t D);
int dpb_cgls_x_step(const float* w, float* delta, float* r, float* p, double* state, double* hist, double tol, int64_t R, int64_t N, int64_t D,
                    void* scratch, size_t scratch_bytes, void* hip_stream);
int dpb_newton_residual(const float* h0, const float* h, const float* u, int nu, const int32_t* dir /*host [n]*/, const float* sign /*host [n]*/,
                        const float* scale /*host [n]*/, double frac, int64_t n, int64_t D, float* res, void* hip_stream);
int dpb_newton_update(const float* x, const float* delta, const double* state /*dev [n][8]*/, double radius, float* x_out,
                      double* step_stats /*dev [n][4]*/, int64_t n, int64_t N, void* hip_stream);
size_t dpb_jac_lstsq_scratch_bytes(const dpb_engine* e, int tap_buf, int nt);
int dpb_jac_lstsq(dpb_engine* e, int tap_buf, const float* c /*dev [nt][N_h]*/, int nt, double mu_abs, double mu_rel, double tol, int iters,
                  float* delta /*dev [nt][N_in]*/, float* resid /*dev [nt][N_h] or NULL*/, double* hist /*dev [iters+1][nt][4]*/, void* scratch,
                  size_t scratch_bytes);
size_t dpb_newton_h_chain_scratch_bytes(const dpb_engine* e, int tap_buf, int n);
int dpb_newton_h_chain(dpb_engine* e, int tap_buf, const float* x /*dev [n][N_in]*/, int n, const float* t /*host [n]*/,
                       const float* ctx /*dev [n][L][Dc] or NULL*/, const float* u /*dev [nu][N_h]*/, int nu, const int32_t* dir,
                       const float* sign, const float* scale /*host [n]*/, int steps, int iters, double mu_abs, double mu_rel, double tol,
                       double radius, int final_shift, float* states /*dev [steps+1][n][N_in]*/, double* hist /*dev [steps][iters+1][n][4]*/,
                       double* step_stats /*dev [steps][n][4]*/, double* shift /*dev [steps+1][n][2]*/, void* scratch, size_t scratch_bytes);

/* ---- the h-space guidance edit (additive to ABI version 1) --------------------------------------------------------------------------
 * The edit_ht == 'h_space_guidance' branch of the global-basis edit jobs (src/modules/edit.py:1232-1245, :1500-1513; the reference calls a
 * h_space_guidance method it never defines), as Kwon et al. state it (Asyrp): a chain carries a state x, a direction c = u[dir] at the tap and a
 * scale sigma; at every DDIM step of the guided interval
 *   e = eps(x, t),  e_s = eps(x, t | h <- h + sigma c)  (a shifted row of dpb_forward_shift),  d = e_s - e,  eP = e + gP d,  eD = e + gD d,
 *   P = (x - eP sqrt(1 - a)) / sqrt(a),   x' = sqrt(a_next) P + sqrt(1 - a_next) eD                                              (eta = 0).
 * (gP, gD) = (1, 0): Asyrp's asymmetric process; (1, 1): the plain DDIM step of the shifted net; any finite pair is accepted.
 *
 * dpb_ddim_step_asym (engine-independent): x, e, e_s [n][N] fp32; out [n][N] (may alias x: every element is read by the thread that overwrites it);
 * x0 [n][N] or NULL receives P; alpha_t, alpha_next, gP, gD host scalars; stats [n][2] FP64 on the device = (sum d^2, flag).  fp32 arithmetic in
 * exactly the operation order of dpb_ddim_step (square roots in fp32 of the fp32 alphas); d, eP and eD are each formed first with one rounding
 * (eP = fma(gP, d, e)), so a row with d == 0 or gP == gD == 0 equals dpb_ddim_step on (x, e) bit for bit.  sum d^2: the fp32 d widened to fp64,
 * per-workgroup partial sums of slices of 4096 elements added in slice order, no atomics -- a function of the row and N only.  A row's results are
 * bitwise the same alone and at any position of a stack, whatever the alignment: rows start at b N floats, and each workgroup takes 16-byte accesses
 * for an aligned row, 4-byte ones otherwise, with the same elements per thread.  A row holding a non-finite value (in x, e or e_s): flag = 1 and NaN
 * in exactly that row of out and x0; no other row changes by a bit.  Two launches per 32768 rows, no host synchronisation.  scratch: 8-byte aligned
 * device memory of >= dpb_ddim_step_asym_scratch_bytes(n, N) bytes (0 when invalid).  Refused (dpb_last_error): null pointers, n < 1, N < 1,
 * non-finite scalars, an alpha outside (0, 1], scratch too small or misaligned.
 *
 * dpb_forward_shift_groups: dpb_forward_shift for `groups` shifted copies of xbatch DIFFERENT samples.  x [xbatch], ctx [xbatch]; the batch has
 * xbatch * groups rows, row r = g * xbatch + b is sample b in group g with its own dir[r] (-1: unshifted) and scale[r] (HOST arrays).  The ops up to
 * the producer of src_buf run ONCE at xbatch; the tap is written as `groups` shifted copies of its xbatch rows; the first xbatch samples of every
 * buffer the rest of the pass still reads (the set of dpb_forward_shift, derived from the tape) are copied as one block to each other group in one
 * launch; the ops after the tap run at xbatch * groups.  groups = 1 is dpb_forward_shift(xbatch = batch) bit for bit, xbatch = 1 its shared-prefix
 * call bit for bit (both take that call's own launches).  State rules and synchronisation of dpb_forward_shift.  Refused: xbatch < 1, groups < 1 or
 * above 64, xbatch * groups > max_batch, nu < 1, a dir[r] outside [-1, nu), a non-finite scale[r], the (src_buf, dst_buf) rules of dpb_forward_shift.
 *
 * dpb_hguide_chain: n chains advanced together through `steps` DDIM steps, no host work between the steps.  x [n][N_in] fp32 NCHW; t, alpha_t,
 * alpha_next: HOST arrays of `steps` entries (every chain shares a step's timestep); ctx [n][L][Dc] or NULL; u [nu][N_h] fp32 NCHW-flattened
 * directions of tap_buf; dir [n] in [0, nu) and scale [n]: HOST arrays.  eps_buf: the network's output buffer (the shape of x).  states
 * [steps + 1][n][N_in]: states[0] = x (states may start at x); step j is one dpb_forward_shift_groups pass with groups = 2 at states[j] and t[j] through
 * to eps_buf -- group 0 unshifted (dir = -1), group 1 the chains' shifts -- and dpb_ddim_step_asym into states[j + 1]; delta [steps][n][2] FP64: its
 * stats.  Host synchronisation: ONE for the call -- the sinusoid rows of ALL the steps are built on the host at entry and uploaded in one copy into
 * scratch; each step moves its row into the time-embedding buffer on the device.  No device allocation: scratch is 256-byte aligned device memory
 * of >= dpb_hguide_chain_scratch_bytes(e, n, steps) bytes (0 when invalid).  The call leaves no primal state, as dpb_forward.  Classifier-free
 * guidance is not part of the chain.  Refused (dpb_last_error; the next call is unaffected): 2n > max_batch, n < 1, steps < 1, nu < 1, a dir[b]
 * outside [0, nu), a non-finite t[j], scale[b], gP or gD, an alpha outside (0, 1], a tap that is not an x-dependent activation, eps_buf not
 * downstream of it or not of the input's shape, a missing ctx, scratch too small or misaligned. */
size_t dpb_ddim_step_asym_scratch_bytes(int64_t n, int64_t N);   /* 0 when invalid */
int dpb_ddim_step_asym(const float* x, const float* e, const float* e_s, float* out, float* x0 /*or NULL*/, int64_t n, int64_t N, float alpha_t,
                       float alpha_next, float gP, float gD, double* stats /*dev [n][2]*/, void* scratch, size_t scratch_bytes, void* hip_stream);
int dpb_forward_shift_groups(dpb_engine* e, const float* x, int xbatch, int groups, float t, const float* ctx, int src_buf, const float* u, int nu,
                             const int32_t* dir /*host [xbatch*groups]*/, const float* scale /*host [xbatch*groups]*/, int dst_buf, int channels,
                             float* out);
size_t dpb_hguide_chain_scratch_bytes(const dpb_engine* e, int n, int steps);
int dpb_hguide_chain(dpb_engine* e, int tap_buf, int eps_buf, const float* x /*dev [n][N_in]*/, int n, const float* t /*host [steps]*/,
                     const float* alpha_t /*host [steps]*/, const float* alpha_next /*host [steps]*/, const float* ctx /*dev [n][L][Dc] or NULL*/,
                     const float* u /*dev [nu][N_h]*/, int nu, const int32_t* dir /*host [n]*/, const float* scale /*host [n]*/, float gP, float gD,
                     int steps, float* states /*dev [steps+1][n][N_in]*/, double* delta /*dev [steps][n][2]*/, void* scratch, size_t scratch_bytes);

/* ---- pullback geodesics between two latents (additive to ABI version 1) ---------------------------------------------------------------
 * The shortest path between two latents under the pullback metric G(x) = J(x)^T J(x) of h = get_h(x, t), as a discrete curve
 * P_0 = x_a, P_1 .. P_m, P_{m+1} = x_b at ONE timestep: the m interior points move, the end points are fixed.  With h_i the tap activation of P_i,
 *   E = 1/2 sum_{i=0..m} ||h_{i+1} - h_i||^2 + 1/2 lambda sum_{i=0..m} ||P_{i+1} - P_i||^2                                   (lambda >= 0)
 *   g_i = J(P_i)^T c_i + lambda d_i,   c_i = 2 h_i - h_{i-1} - h_{i+1},   d_i = 2 P_i - P_{i-1} - P_{i+1}                   (i = 1 .. m)
 * and one iteration is the Jacobi step P_i <- P_i - eta g_i, every g_i taken from the same old curve.  lambda = 0 is well posed for this descent:
 * g_i lies in the row space of J, so what J does not see of the start curve is kept.  (The reference has no such job; its paper's metric is this G.)
 *
 * dpb_geodesic_cotangents (engine-independent): h [m+2][D] fp32, cot [m][D] fp32, seg [m+1] FP64, csq [m] FP64 or NULL, all on the device.
 *   cot_i = fl32((2 h_i - h_{i-1}) - h_{i+1}) (row i - 1 of cot), formed in fp64 and rounded once; seg_i = sum (h_{i+1} - h_i)^2 in fp64 (fp32 widened
 *   on load, the difference, its square and the sum each rounded once; per-workgroup partial sums of slices of 4096 elements, added in slice order);
 *   csq_i = sum cot_i^2 of the ROUNDED cotangent, the same chain (row i - 1 of csq): the ||c_i||^2 of the step rule eta_0 = 1/4 sum ||c_i||^2 /
 *   sum ||g_i||^2.  No atomics: cot_i, csq_i and seg_i are a function of rows i-1 .. i+1 and D only -- bitwise the same in any longer curve and at any
 *   alignment (16-byte accesses for an aligned row, 4-byte ones otherwise, the same elements per thread).  Two launches, no host synchronisation.
 * dpb_geodesic_update (engine-independent): P [m+2][N], W [m][N] (the adjoint results J^T c), P_out [m+2][N] fp32; eta, lambda host scalars;
 *   stats [m][4] FP64, xseg [m+1] FP64 on the device.  Interior rows: g = W_i + lambda ((2 P_i - P_{i-1}) - P_{i+1}) and P_out_i = fl32(P_i - eta g),
 *   in fp64, every operation rounded once and one rounding to fp32; the end rows are copied.  eta == 0 hands P through bit for bit.  P_out must not
 *   overlap P (a row reads its neighbours' OLD values): refused.  stats[i - 1] = (sum W_i^2, sum g_i^2, sum (P_out_i - P_i)^2, flag) and xseg_i =
 *   sum (P_{i+1} - P_i)^2 of the OLD curve, the fixed-order fp64 slice sums of above.  A row whose W_i, P_i or neighbours P_{i-1}, P_{i+1} hold a
 *   non-finite value: flag = 1 and NaN in exactly that row of P_out (its sums are those of its elements as they are); no other row changes by a bit.
 *   Two launches, no host synchronisation.
 * Either: scratch is 8-byte aligned device memory of >= its *_scratch_bytes(m, D or N) bytes (0 when invalid).  Refused (dpb_last_error), the outputs
 * untouched: null pointers (csq may be NULL), m < 1 or m + 2 > 32768, a row length < 1, a non-finite eta or lambda, lambda < 0, scratch too small or
 * misaligned.
 *
 * dpb_geodesic_chain: `iters` Jacobi iterations with no host work between them.  P [m+2][N_in] fp32 NCHW, one timestep t, ctx [m+2][L][Dc] or NULL.
 * curves [iters + 1][m+2][N_in]: curves[0] = P (curves may start at P).  At entry the two END POINTS run once to the tap as one batch of 2; their
 * activations stay in scratch as fp32 NCHW for the whole call.  Iteration j: one primal pass of the m interior rows of curves[j] up to the tap, its
 * activations converted into the middle of the [m+2][N_h] block, dpb_geodesic_cotangents (seg_h[j]), the adjoint pass of dpb_vjp with one cotangent
 * per sample, dpb_geodesic_update into curves[j + 1] (stats[j], seg_x[j]).  seg_h, seg_x [iters + 1][m+1], stats [iters][m][4] FP64; csq [iters][m]
 * FP64 or NULL: the csq of the cotangent kernel at every iteration (||c_i||^2 is no function of the segment sums, and the step rule needs it).  Row `iters` of
 * seg_h / seg_x takes one more forward pass of the interior rows when final_energy != 0, else it is NaN.  So E of curves[j] is
 * 1/2 sum seg_h[j] + 1/2 lambda sum seg_x[j].
 * Host synchronisation: ONE for the call -- the upload of the timestep embedding in the end-point pass; it stays resident in the engine for every
 * other pass.  No device allocation: scratch is 256-byte aligned device memory of >= dpb_geodesic_chain_scratch_bytes(e, tap_buf, m) bytes (0 when
 * invalid).  The call leaves no primal state, as dpb_forward.  Refused (dpb_last_error; the next call is unaffected): m outside
 * [1, min(max_batch, max_tangents)], max_batch < 2, iters < 1, a non-finite t, eta or lambda, lambda < 0, a tap that is not an x-dependent
 * activation, a missing ctx, scratch too small or misaligned. */
size_t dpb_geodesic_cotangents_scratch_bytes(int64_t m, int64_t D);   /* 0 when invalid */
int dpb_geodesic_cotangents(const float* h /*dev [m+2][D]*/, float* cot /*dev [m][D]*/, double* seg /*dev [m+1]*/, double* csq /*dev [m] or NULL*/,
                            int64_t m, int64_t D, void* scratch, size_t scratch_bytes, void* hip_stream);
size_t dpb_geodesic_update_scratch_bytes(int64_t m, int64_t N);       /* 0 when invalid */
int dpb_geodesic_update(const float* P /*dev [m+2][N]*/, const float* W /*dev [m][N]*/, float* P_out /*dev [m+2][N]*/, float eta, float lambda,
                        int64_t m, int64_t N, double* stats /*dev [m][4]*/, double* xseg /*dev [m+1]*/, void* scratch, size_t scratch_bytes,
                        void* hip_stream);
size_t dpb_geodesic_chain_scratch_bytes(const dpb_engine* e, int tap_buf, int m);
int dpb_geodesic_chain(dpb_engine* e, int tap_buf, const float* P /*dev [m+2][N_in]*/, int m, float t, const float* ctx /*dev [m+2][L][Dc] or NULL*/,
                       float eta, float lambda, int iters, int final_energy, float* curves /*dev [iters+1][m+2][N_in]*/,
                       double* seg_h /*dev [iters+1][m+1]*/, double* seg_x /*dev [iters+1][m+1]*/, double* stats /*dev [iters][m][4]*/,
                       double* csq /*dev [iters][m] or NULL*/, void* scratch, size_t scratch_bytes);

/* Token + position embedding lookup of the CLIP text encoder behind pipe._encode_prompt (src/modules/edit.py:505-522):
 * out[b][c][t] = tok_table[ids[b][t]][c] + pos_table[t][c], fp32 in the engine's NCHW boundary layout (H*W = tokens),
 * ready for dpb_primal of a text-encoder tape.  Tables are [vocab][channels] / [tokens][channels] in `dtype`. */
int dpb_embed_tokens(const int32_t* ids, const void* tok_table, const void* pos_table, int dtype, float* out, int batch,
                     int tokens, int channels, int vocab, void* hip_stream);

/* Introspection used by tests / bench: number of kernel launches and algorithmic GEMM flops of the last pass.  `launches` is the number of
 * kernels the pass enqueued, counted at the launch itself; memsets and copies are not included. */
int dpb_engine_stats(const dpb_engine* e, int64_t* launches, double* gemm_flops, double* gemm_bytes);
/* Measurement aid (bench.py roofline leg, never on in a timed region): bracket every GEMM launch with HIP
 * events on the engine's stream; _read synchronises and sums the launches of one GEMM kernel kind: count, total
 * milliseconds, algorithmic flops.  kind (for products: the `kind` column of the tile table, kernels.h): 0 register-staged 64x64, 1 register-staged 128x128, 2 BK=32 ring 128x128 /
 * 256x128, 3 BK=32 ring 64x64, 4 BK=64 ring with 128-column tiles (gemm_ring64.hip), 5 halo-tile 3x3 convolution (gemm_halo.hip), 6 BK=64 ring
 * with the 256x256 tile, 11 the 8-phase 256x256 tile (gemm_p8.hip: two wave groups alternating between load and matrix segments, counted vmcnt), 12 the
 * weights-resident streaming kernel of the K = 320 linear layers (gemm_wres.hip: weight slice in registers, activation rows streamed through an LDS ring);
 * attention (algorithmic flops = 2 / 5 / 7 L x L x d products per head and sample / tangent / cotangent): 7 flash forward,
 * 8 fused self-attention tangent, 9 fused self-attention adjoint (its query-major and key-major launches in ONE bracket; the CSV's `gather`
 * column holds the route: bit 0 multi-cotangent query-major kernel, bit 1 shared-probability key-major kernel), 10 one-launch cross-attention
 * tangent (gather 0) / adjoint (gather 1): 2 L x 77 x d products.  kind + 1000 returns the RAW bracket times of that kind (without the empty-bracket
 * correction of dpb_engine_profile_overhead, which clamps a bracket shorter than the correction to 0); any other kind (neither 0..12 nor 1000..1012) fails.
 * _dump writes one CSV line per recorded bracket. */
int dpb_engine_profile(dpb_engine* e, int enable);
int dpb_engine_profile_read(dpb_engine* e, int kind, int64_t* count, double* total_ms, double* flops);
int dpb_engine_profile_dump(dpb_engine* e, const char* csv_path);
/* The per-launch times of _read / _dump are event-bracket times minus a calibrated empty-bracket time (measured when profiling is switched on);
 * this returns that correction so that the raw bracket times can be reconstructed (raw = reported + overhead per launch). */
int dpb_engine_profile_overhead(const dpb_engine* e, double* bracket_overhead_ms);
/* Tuning overrides for micro-benchmarks and the bitwise kernel-equivalence tests (0 / -1 = heuristic): "gemm_tile"
 * (the forced code of one row of the tile table kGemmTiles in diffusion_pullback_amd/csrc/kernels.h -- the ONE list of every tile the library launches:
 * family, plan code, forced code, block geometry, stages, waves, profile kind, capabilities, and the substitute row that runs a product the forced tile
 * does not take; a value that names no row leaves the heuristic in charge, with the halo-tile convolution off), "gemm_splitk" (n), "gemm_kch", "p8" (1, default: the dispatch may pick the 8-phase tile; 0 = the ring / halo dispatch of round 4), "wres" (1, default: K = 320 / N % 320 == 0 plain products go to the weights-resident kernel from 49 152 rows (N = 320) / 147 456 rows (wider N) on; 0 = the round-5 dispatch; bitwise equal), "halo_loop" (1, default: the halo-tile convolution runs its 8-phase main loop; 0 = its ring loop, also DPB_HALO_LOOP=0; bitwise equal), "gemm_dma_auto" (0|1), "gemm_order" (-1 | 0 A-major | 1 B-major block
 * order per XCD), "gn_deterministic" (1, default: GroupNorm statistics of the two-pass kernels reduced in a fixed order -> bitwise
 * reproducible runs; 0 = the round-1 atomic statistics, A/B only), "graph_iterate" (0|1: dpb_pullback_iterate replays a captured hipGraph on a non-default stream;
 * measured equal to eager launches, default 0), "attn_shared" (2, default: shared-probability key-major adjoint of the head-dim-40
 * self-attention layers; 0 = the per-cotangent kernel of round 2; 6 = also route head dim 64 (SD-2.x) through the shared-probability adjoint kernels, measured
 * no faster there), "lazy_reduce" (1, default: a split-K product consumed by a one-launch GroupNorm or a
 * LayerNorm leaves its fp32 slabs to that kernel instead of running splitk_reduce_kernel; 0 = always reduce; bitwise the same results),
 * "ln_fuse" (0, default since round 6: separate launches; 1 = LayerNorm in the epilogue of the 320-wide products), "cross_primal" (1, default: the forward of a text-conditioned attention layer is
 * ONE launch; 0 = GEMM + softmax + transpose + GEMM), "cross_fold" (also DPB_CROSS_FOLD.  The tangent / adjoint of a text-conditioned attention layer with its to_q and
 * to_out products as TWO products: the sample's constant K / V are multiplied into the weights by the stashing primal pass, the softmax Jacobian is the epilogue of the
 * first product.  1, default: where the folded products cost no more MACs than the chain -- 208 heads C <= 2 C^2 + 384 C, one sample; 0 = off; 2 = wherever the tape allows it;
 * v > 2 = as 1 for layers of at least v channels), "geglu_fwd" (1, default: dpb_forward applies GEGLU in the epilogue of the unsplit FF-in products), "iter_alias" (1, default: inside dpb_pullback_iterate the tap's
 * tangent passes from the tangent to the adjoint pass on the device, U is written by the last iteration only; 0 = fp32 round trip through U every iteration; bitwise equal).
 * Environment, read once per process (tuning / ablation only): DPB_GEMM_OVERRIDE="MxNxK:gather=code/split,..." forces
 * kernel and split count per product shape; DPB_P8 (0: no 8-phase tile), DPB_WRES (0: no weights-resident kernel), DPB_WRES_MIN_M, DPB_TILE256, DPB_CONV_HALO, DPB_SPLITK_TARGET, DPB_GEMM_ORDER, DPB_GN_FUSED, DPB_GN_BLOCKS,
 * DPB_GN_DETERMINISTIC, DPB_LN_ROWS, DPB_LN_FUSE, DPB_LAZY_REDUCE, DPB_ATTN_WAVES, DPB_ATTN_MULTI, DPB_ATTN_SHARED, DPB_ATTN_XCD, DPB_FUSED_ATTN_MIN_L,
 * DPB_NO_FUSED_ATTN, DPB_NO_CROSS_ATTN, DPB_NO_GEGLU_FUSE switch individual kernels / fusions off or pick their variants; DPB_EIG_PAR (0: the one-wave cyclic
 * eigen-solve of rounds 1-5 for every k <= 56, 2: the round-robin one for every k), DPB_ORTH_BATCH (0: the samples of a batch re-orthonormalised one by one); DPB_GEMM_TRACE=1 prints every
 * product and synchronises after it (debugging). */
int dpb_debug_set(const char* key, int value);

/* Introspection for the tests of the folded text-conditioned attention route ("cross_fold" below; additive to ABI version 1).  index counts the
 * attention layers of the tape that CAN take the route (constant K / V on the one-launch cross route, 16-bit engine, to_q and to_out products
 * private to the layer); past the last one the call fails.  info[12] = {op index, 1 if the last dpb_primal built the folded operands, C, heads,
 * query rows, keys, and the workspace byte offsets of Gt [heads 128][C], Gk [C][heads 80], F [heads 128][C], Fk [C][heads 80] (engine dtype),
 * the fp32 probabilities [rows][heads][80] and the scratch [nt rows][heads 80] the first folded product of a pass writes}. */
int dpb_debug_cross_fold(const dpb_engine* e, int index, int64_t* info);

/* Host-only (no GPU work): the launch plan the GEMM dispatch picks for a product C[M][N] = A[M][K] B[N][K]^T -- plain rows (conv_hw = 0) or
 * a 3x3 / stride 1 / pad 1 convolution on conv_hw x conv_hw images of conv_cin channels (K = 9 conv_cin) -- with `slab_bytes` of split-K
 * scratch.  kind: 0 / 1 register-staged 64x64 / 128x128 tile, 2 asynchronous kernel (LDS rings, 8-phase tile, weights-resident kernel), 3 halo-tile
 * convolution; tile: the plan code of its row in the tile table (kernels.h; see dpb_debug_set); epilogue 0 plain, 1 / 2 / 5 fused GEGLU tangent / adjoint / forward.  splitk x M x N x 4 bytes never exceeds slab_bytes.  Lets the
 * dispatch rules be tested on a machine without a GPU (tests/test_host_logic.py). */
int dpb_debug_gemm_plan(int dtype, int M, int N, int K, int conv_hw, int conv_cin, int epilogue, int64_t slab_bytes, int* kind, int* tile,
                        int* splitk);

#ifdef __cplusplus
}
#endif
#endif /* DPB_H */
