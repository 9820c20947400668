"""Numpy float64 restatement of the Grassmann Frechet (Karcher) mean, in the AMBIENT space on purpose: bases are orthonormalised by QR, the log map
comes from the SVD of Y Q_i^T, the exp map from the thin SVD of the mean tangent, and a QR follows every step -- none of the coefficient / Gram
algebra of csrc/frechet.hip.  Same init, step and stop rule as geometry.frechet_mean, and the `weight` ordering of its finish.

Also the constructions with known answers that tests/test_frechet_host.py holds this file to and tests/test_gpu_frechet.py runs on the GPU."""
import numpy as np
from scipy.linalg import subspace_angles

DOMAIN = np.pi / 2 - 1e-6


def orthonormal_rows(a):
    """a [k, N] -> Q [k, N] with orthonormal rows spanning the rows of a"""
    q, _ = np.linalg.qr(np.asarray(a, dtype=np.float64).T)
    return q.T


def log_map(y, q):
    """Log_Y(span Q) as a [k, N] tangent at Y (rows orthonormal), and the principal angles (ascending).  With Y Q^T = U cos W^T the rows of
    D = W^T Q - cos U^T Y are orthogonal with norms sin(theta): the tangent is U diag(theta / sin) D."""
    u, c, wt = np.linalg.svd(y @ q.T)
    d = wt @ q - c[:, None] * (u.T @ y)
    s = np.linalg.norm(d, axis=1)
    th = np.arctan2(s, c)
    scale = np.divide(th, s, out=np.zeros_like(s), where=s > 0)
    return u @ (scale[:, None] * d), th


def exp_map(y, t, tau=1.0):
    """Exp_Y(tau T), rows re-orthonormalised by QR"""
    p, sig, zt = np.linalg.svd(t, full_matrices=False)
    yn = p @ (np.cos(tau * sig)[:, None] * (p.T @ y)) + p @ (np.sin(tau * sig)[:, None] * zt)
    return orthonormal_rows(yn)


def angles_to(y, q):
    """principal angles of the row span of Y to that of Q, descending (scipy, float64).  Both are first written in an orthonormal basis of their joint
    span (the R factor of one QR of [Y^T Q^T]): an isometry, so the angles are the same, and scipy's own orthonormalisation then works on 2k x k
    matrices, not N x k."""
    y, q = np.asarray(y, np.float64), np.asarray(q, np.float64)
    r = np.linalg.qr(np.concatenate([y, q]).T, mode="r")
    return subspace_angles(r[:, :len(y)], r[:, len(y):])


def max_angle(y0, y1):
    return float(angles_to(y0, y1)[0])


def frechet_mean_ref(a, init=0, max_iter=1000, tol=1e-6, step=1.0):
    """a [B, k, N] -> (Y [k, N] float64 in canonical order, info) with info as geometry.frechet_mean returns it (numpy arrays)."""
    a = np.asarray(a, dtype=np.float64)
    b, k, _ = a.shape
    qs = [orthonormal_rows(x) for x in a]
    y = qs[init].copy()
    cost, ghist, converged = [], [], False
    iters = 0
    while True:
        logs = [log_map(y, q) for q in qs]
        cost.append(0.5 * np.mean([np.sum(th ** 2) for _, th in logs]))
        worst = [i for i, (_, th) in enumerate(logs) if th.max() > DOMAIN]
        if worst:
            raise ValueError(f"basis {worst[0]} left the log map's domain at step {iters}")
        if iters >= max_iter:
            break
        t = np.mean([l for l, _ in logs], axis=0)
        g = float(np.linalg.norm(t))
        ghist.append(g)
        if g < tol:
            converged = True
            break
        y = exp_map(y, t, step)
        iters += 1
    wm = np.mean([(y @ q.T) @ (q @ y.T) for q in qs], axis=0)
    lam, v = np.linalg.eigh(wm)
    order = np.argsort(-lam, kind="stable")
    y = v[:, order].T @ y
    theta = np.stack([angles_to(y, q) for q in qs])
    return y, {"iterations": iters, "converged": converged, "grad_norm": ghist[-1] if ghist else float("nan"), "cost": np.array(cost),
               "grad_norm_history": np.array(ghist), "weight": lam[order], "theta": theta}


# ------------------------------------------------------------------------------------------------------------ sets with known answers
def random_orthonormal(rng, k, n):
    return orthonormal_rows(rng.standard_normal((k, n)))


def mixing(rng, k, cond=100.0):
    """a k x k matrix of condition number cond (1 for k = 1): random orthogonal factors around log-spaced singular values"""
    if k == 1:
        return np.array([[1.7]])
    u, _ = np.linalg.qr(rng.standard_normal((k, k)))
    v, _ = np.linalg.qr(rng.standard_normal((k, k)))
    return (u * np.logspace(0, -np.log10(cond), k)) @ v.T


def clustered_set(rng, b, k, n, spread=0.2, cond=30.0):
    """b non-orthonormal bases of k rows around one random subspace: row perturbations of norm ~ spread, rows mixed by a matrix of condition cond;
    float32, as the GPU sees them"""
    q0 = random_orthonormal(rng, k, n)
    out = []
    for _ in range(b):
        m = q0 + spread * rng.standard_normal((k, n)) / np.sqrt(n)
        out.append(mixing(rng, k, cond) @ m)
    return np.stack(out).astype(np.float32)


def spread_set(rng, b=6, k=6, n=2048):
    """b random k-dimensional subspaces of R^n (principal angles near pi/2: a slowly converging set)"""
    return np.stack([rng.standard_normal((k, n)) for _ in range(b)]).astype(np.float32)


def tangent_at(rng, y, norm2):
    """a random tangent at Y (rows orthogonal to the rows of Y) of spectral norm norm2: the largest principal angle of Exp_Y(+-T) to Y"""
    h = rng.standard_normal(y.shape)
    h -= (h @ y.T) @ y
    return h * (norm2 / np.linalg.svd(h, compute_uv=False)[0])


def plus_minus_set(rng, k, n, norms=(0.3, 0.6)):
    """(members [2 len(norms), k, N] float32, Y* [k, N]): the pairs Exp_{Y*}(+-D_j) with ||D_j||_2 in norms -- their logs at Y* cancel, and 0.6 is inside
    the convexity radius pi/4, so the mean is Y*"""
    ystar = random_orthonormal(rng, k, n)
    members = []
    for nm in norms:
        d = tangent_at(rng, ystar, nm)
        members += [exp_map(ystar, d), exp_map(ystar, -d)]
    return np.stack(members).astype(np.float32), ystar


def pair_set(rng, k, n, angle=0.5):
    """two bases whose principal angles are all <= angle: the mean is the geodesic midpoint, at half the pair's angles from each"""
    y0 = random_orthonormal(rng, k, n)
    y1 = exp_map(y0, tangent_at(rng, y0, angle))
    return np.stack([y0, y1]).astype(np.float32)


def quantised(a, bits=10):
    """the entries rounded to multiples of 2^-bits, so that remix() below is exact in float32"""
    return (np.round(np.asarray(a, np.float64) * 2.0 ** bits) / 2.0 ** bits).astype(np.float32)


def remix(a):
    """every basis's rows mixed by D (4 I + S): S the skew matrix with +1 above and -1 below the diagonal (singular values of 4 I + S within
    [4, sqrt(20)]), D = diag(1, 2, 4, .., 64, 1, ..) rotated by the basis's index -- condition number <= 64 sqrt(20) / 4 = 72.  Integer entries up to 2^8
    and three terms per row: on entries that are multiples of 2^-10 below 1 the products and sums are exact in float32, so the spans do not move at all."""
    a = np.asarray(a, np.float64)
    b, k, _ = a.shape
    out = []
    for i in range(b):
        m = 4.0 * np.eye(k) + np.diag(np.ones(k - 1), 1) - np.diag(np.ones(k - 1), -1)
        d = 2.0 ** ((np.arange(k) + i) % 7)
        out.append((d[:, None] * m) @ a[i])
    out = np.stack(out)
    assert np.array_equal(out, out.astype(np.float32).astype(np.float64)), "remix() must be exact in float32: pass quantised() members"
    return out.astype(np.float32)
