"""Numpy float64 reference of the flag (extrinsic, chordal) mean, in the AMBIENT space on purpose: every member is orthonormalised by QR, the stacked
Q's go through one SVD, and the mean is the top right singular vectors with sigma^2 / B -- none of the Gram / coefficient algebra of
csrc/flagmean.hip.  Angles by scipy.

Also a numpy restatement of the kernel's own method (block subspace iteration with a Rayleigh-Ritz step on the whitened Gram), the "graded" sets of
the tests, and the Karcher iteration of tests/_frechet_ref.py started at a given point."""
import numpy as np

import _frechet_ref as F
from _frechet_ref import angles_to, clustered_set, max_angle, mixing, orthonormal_rows, quantised, random_orthonormal, remix, spread_set  # noqa: F401


def flag_mean_ref(a, r=None):
    """a [B, k, N] -> (Y [r, N] float64, info): weight [r], eigenvalues (all min(R, N) of them, descending), theta [B, min(r, k)] descending"""
    a = np.asarray(a, dtype=np.float64)
    b, k, _ = a.shape
    r = k if r is None else r
    qs = [orthonormal_rows(x) for x in a]
    _, s, vt = np.linalg.svd(np.concatenate(qs), full_matrices=False)
    y = vt[:r]
    w = s ** 2 / b
    theta = np.stack([angles_to(y, q) for q in qs])
    return y, {"weight": w[:r], "eigenvalues": w, "theta": theta}


def rel_gaps(w):
    """g[j - 1] = (w_{j-1} - w_j) / w_{j-1}: the relative gap after row j (1-based count of rows kept), 1.0 after the last eigenvalue"""
    w = np.asarray(w, np.float64)
    nxt = np.append(w[1:], 0.0)
    return (w - nxt) / np.maximum(w, 1e-300)


def rayleigh_weights(a, y):
    """mean_i ||Q_i y_j||^2 of the rows of y: what `weight` must be for any orthonormal Y, converged or not"""
    qs = [orthonormal_rows(x) for x in np.asarray(a, np.float64)]
    y = np.asarray(y, np.float64)
    return np.mean([np.sum((q @ y.T) ** 2, axis=0) for q in qs], axis=0)


def block_width(R, r):
    return int(min(64, R, (r + 8 + 15) // 16 * 16))


def _orth_gram(p, symmetric, drop=1e-13):
    d, v = np.linalg.eigh(p.T @ p)
    dinv = np.where(d > drop * d.max(), 1.0 / np.sqrt(np.maximum(d, 1e-300)), 0.0)
    return p @ ((v * dinv) @ v.T if symmetric else v * dinv)


def flag_mean_method(a, r=None, max_iter=1000, tol=1e-12, seed=0):
    """the kernel's method restated: Ghat from the QR'd members, a block of m columns, per iteration W = Ghat Z, T = Z^T W = S L S^T, the residual
    max_{j<r} ||(W S)_j - l_j (Z S)_j|| / l_0, Z <- orth(W S) through the Gram's eigen-decomposition, twice; the finish is the ambient-space
    Rayleigh-Ritz step of the pencil (W^T W, Z^T W).  The start block is numpy's, not the kernel's: only the method is restated."""
    a = np.asarray(a, dtype=np.float64)
    b, k, _ = a.shape
    r = k if r is None else r
    q = np.concatenate([orthonormal_rows(x) for x in a])
    g = q @ q.T
    R = b * k
    m = block_width(R, r)
    if m == R:
        z = np.eye(R)
    else:
        z = np.random.default_rng(seed).uniform(-1, 1, (R, m))
        z = _orth_gram(_orth_gram(z, True), True)
    iters, converged, res = 0, False, float("nan")
    while iters < max_iter:
        w = g @ z
        t = z.T @ w
        lam, s = np.linalg.eigh((t + t.T) / 2)
        order = np.argsort(-lam, kind="stable")
        lam, s = lam[order], s[:, order]
        ws, zs = w @ s, z @ s
        res = np.linalg.norm(ws[:, :r] - lam[:r] * zs[:, :r], axis=0).max() / lam[0]
        iters += 1
        if res <= tol:
            converged = True
            break
        z = _orth_gram(_orth_gram(ws, False), True)
    # the finish: Rayleigh-Ritz in the ambient space over the rows Z^T Q -- the pencil (W^T W, T), whitened by T's eigen-decomposition
    w = g @ z
    t = z.T @ w
    lam, s = np.linalg.eigh((t + t.T) / 2)
    linv = np.where(lam > 1e-13 * lam.max(), 1.0 / np.sqrt(np.maximum(lam, 1e-300)), 0.0)
    sl = s * linv
    mu, u = np.linalg.eigh(sl.T @ (w.T @ w) @ sl)
    order = np.argsort(-mu, kind="stable")
    mu, u = mu[order], u[:, order]
    c = (z @ sl @ u[:, :r]).T
    return c @ q, {"iterations": iters, "converged": converged, "residual": res, "weight": mu[:r] / b, "eigenvalues": mu / b}


def graded_set(rng, b, k, n, noise=(0.1, 0.45, 0.87), cond=30.0):
    """b bases of k rows: len(noise) shared directions, direction j perturbed per member by a vector of norm ~ noise[j] (the members hold it with
    cos^2 ~ 1 / (1 + noise_j^2)), plus k - len(noise) private random rows, the rows mixed by a matrix of condition cond; float32"""
    s = len(noise)
    assert s <= k
    shared = random_orthonormal(rng, s, n)
    out = []
    for _ in range(b):
        rows = shared + np.asarray(noise)[:, None] * rng.standard_normal((s, n)) / np.sqrt(n)
        rows = np.concatenate([rows, rng.standard_normal((k - s, n)) / np.sqrt(n)])
        out.append(mixing(rng, k, cond) @ rows)
    return np.stack(out).astype(np.float32)


def domain_set(rng, k=3, n=64):
    """four orthonormal bases: member 1 is member 0 with its last row turned by pi/2, members 2 and 3 have it turned by 0.5 and 1.0 rad -- the Karcher
    iteration cannot start at member 0 (member 1 is at the cut locus) but the flag mean is 0.25 .. 0.82 rad from every member"""
    f = random_orthonormal(rng, k + 1, n)
    out = []
    for ang in (0.0, np.pi / 2, 0.5, 1.0):
        m = f[:k].copy()
        m[k - 1] = np.cos(ang) * f[k - 1] + np.sin(ang) * f[k]
        out.append(m)
    return np.stack(out).astype(np.float32)


def karcher_from(a, y0, max_iter=1000, tol=1e-6, step=1.0):
    """the iteration of _frechet_ref.frechet_mean_ref started at the span of y0: (Y, steps, converged)"""
    qs = [orthonormal_rows(x) for x in np.asarray(a, np.float64)]
    y = orthonormal_rows(y0)
    for it in range(max_iter + 1):
        logs = [F.log_map(y, q) for q in qs]
        if any(th.max() > F.DOMAIN for _, th in logs):
            raise ValueError(f"a basis left the log map's domain at step {it}")
        t = np.mean([l for l, _ in logs], axis=0)
        if np.linalg.norm(t) < tol:
            return y, it, True
        if it == max_iter:
            break
        y = F.exp_map(y, t, step)
    return y, max_iter, False
