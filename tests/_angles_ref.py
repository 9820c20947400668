"""Float64 restatement of dpb_subspace_angles (diffusion_pullback_amd/csrc/angles.hip) and the crafted inputs its tests share.

The restatement follows the kernel step by step -- Gram of all rows, row normalisation through the Gram diagonal, Cholesky whitening of each basis's
own block, M = L_i^-1 Ghat_ij L_j^-T, eigenvalues of S = I - M M^T, theta = asin(sqrt(l)) for l <= 1/2 else acos(sqrt(1 - l)) -- in numpy float64.
tests/test_subspace_angles_host.py holds it to scipy.linalg.subspace_angles at the bar the GPU tests use, so the bar is re-measured on every run.
"""
import numpy as np

BAR = 1e-6                       # rad per angle against scipy.linalg.subspace_angles (float64, the same fp32 inputs); dist: relative
MIN_PIVOT = 1e-10                # ANGLES_MIN_PIVOT of angles.hip
SHAPES_HOST = [(5, 4096), (50, 16384), (17, 3001)]
SHAPES_GPU = [(1, 7), (4, 4), (5, 4096), (16, 2048), (17, 3001), (50, 16384), (128, 2048)]
VARIANTS = ["plain", "mixed", "scaled"]
FIXED_ANGLES = [0.0, 1e-6, 1e-4, 1e-2, np.pi / 2 - 1e-3, np.pi / 2]


def crafted(k, N, variant, seed=0):
    """A, B [k][N] float32 with known principal angles: q, p from the QR of a seeded N x 2k Gaussian matrix (N x N when 2k > N: the two spans then
    cannot be placed at chosen angles -- for k = N both are the whole space), A = q, B = cos(theta) q + sin(theta) p, theta = the fixed angles
    (as many as fit) and uniform draws.  'mixed': both bases times a random k x k matrix orthogonal . (I + 0.05 G) (condition number of a few
    units); 'scaled': the same, then row scales spread over 1 .. 100."""
    rng = np.random.default_rng(1000 * k + N + seed)
    cols = min(2 * k, N)
    Q, _ = np.linalg.qr(rng.standard_normal((N, cols)))
    q = Q[:, :k].T
    theta = np.concatenate([FIXED_ANGLES, rng.uniform(0.0, np.pi / 2, max(0, k - len(FIXED_ANGLES)))])[:k]
    if cols == 2 * k:
        p = Q[:, k:].T
        A, B = q, np.cos(theta)[:, None] * q + np.sin(theta)[:, None] * p
    else:                                       # no room for a second k-frame orthogonal to the first
        A, B = q, np.linalg.qr(rng.standard_normal((N, k)))[0].T
    if variant in ("mixed", "scaled"):
        for name in ("A", "B"):
            O, _ = np.linalg.qr(rng.standard_normal((k, k)))
            mix = O @ (np.eye(k) + 0.05 * rng.standard_normal((k, k)))
            if name == "A":
                A = mix @ A
            else:
                B = mix @ B
    if variant == "scaled":
        A = np.exp(rng.uniform(0.0, np.log(100.0), k))[:, None] * A
        B = np.exp(rng.uniform(0.0, np.log(100.0), k))[:, None] * B
    return np.ascontiguousarray(A, dtype=np.float32), np.ascontiguousarray(B, dtype=np.float32)


def scipy_angles(A, B):
    """scipy.linalg.subspace_angles of the row spans, float64, descending"""
    from scipy.linalg import subspace_angles
    return subspace_angles(np.asarray(A, dtype=np.float64).T, np.asarray(B, dtype=np.float64).T)


def _whiten(G):
    """W = L^-1 D^-1/2 of one basis's Gram block, or None for a degenerate basis"""
    d = np.diag(G)
    if not (np.all(d > 0) and np.all(np.isfinite(d))):
        return None
    rs = 1.0 / np.sqrt(d)
    Gh = G * rs[:, None] * rs[None, :]
    k = G.shape[0]
    L = np.zeros((k, k))
    for j in range(k):                          # the pivot rule of the kernel, which numpy's cholesky does not expose
        piv = Gh[j, j] - L[j, :j] @ L[j, :j]
        if not piv >= MIN_PIVOT:
            return None
        L[j, j] = np.sqrt(piv)
        L[j + 1:, j] = (Gh[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return np.linalg.solve(L, np.eye(k)) * rs[None, :]


def ref_angles(A, B=None):
    """theta [Ba][Bb][k] (descending) and dist [Ba][Bb] of stacks A [Ba][k][N], B [Bb][k][N] (None: self mode), float64; NaN rows / columns for
    degenerate bases, an exactly zero self-mode diagonal"""
    A = np.asarray(A, dtype=np.float64)
    self_mode = B is None
    B = A if self_mode else np.asarray(B, dtype=np.float64)
    Ba, k, _ = A.shape
    Bb = B.shape[0]
    Wa = [_whiten(a @ a.T) for a in A]
    Wb = Wa if self_mode else [_whiten(b @ b.T) for b in B]
    theta = np.full((Ba, Bb, k), np.nan)
    for i in range(Ba):
        for j in range(Bb):
            if Wa[i] is None or Wb[j] is None:
                continue
            if self_mode and i == j:
                theta[i, j] = 0.0
                continue
            if self_mode and i > j:
                theta[i, j] = theta[j, i]
                continue
            M = Wa[i] @ (A[i] @ B[j].T) @ Wb[j].T
            lam = np.clip(np.linalg.eigvalsh(np.eye(k) - M @ M.T), 0.0, 1.0)[::-1]
            theta[i, j] = np.where(lam <= 0.5, np.arcsin(np.sqrt(lam)), np.arccos(np.sqrt(np.clip(1.0 - lam, 0.0, 1.0))))
    return theta, np.sqrt((theta ** 2).sum(-1))
