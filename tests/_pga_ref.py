"""Numpy float64 restatement of principal geodesic analysis (tangent PCA) of subspaces, in the AMBIENT space on purpose: every member is orthonormalised by
QR, its log map at the base comes from _frechet_ref.log_map (an SVD of Y Q_i^T), the B tangents are flattened, centred and handed to ONE SVD, and the
covariate fit is numpy.linalg.lstsq on the flattened tangents -- none of the coefficient / Gram algebra of csrc/pga.hip.  Same sign rule, ordering and
definitions as geometry.grassmann_pga.

Also the planted sets tests/test_pga_host.py holds this file to and tests/test_gpu_pga.py runs on the GPU, and `tangent_gram_identity`: the k x k
restatement of the tangent Gram that the pair kernel evaluates, kept here so that the host test can hold it to the ambient Gram."""
import numpy as np

import _frechet_ref as F


def polar_rows(y):
    """the orthonormal rows closest to the rows of y (the polar factor): fp32-rounded orthonormal rows made orthonormal in float64 without moving them"""
    y = np.asarray(y, np.float64)
    lam, v = np.linalg.eigh(y @ y.T)
    return (v / np.sqrt(lam)) @ v.T @ y


def logs_at(y, a):
    """(L [B, k, N], theta [B, k] descending): the log maps at Y (orthonormal rows) of the row spans of a [B, k, N]; row j of L_i is the image of row j of Y"""
    ls, ths = [], []
    for x in np.asarray(a, np.float64):
        l, _ = F.log_map(y, F.orthonormal_rows(x))
        ls.append(l)
        ths.append(F.angles_to(y, x))
    return np.stack(ls), np.stack(ths)


def fix_signs(scores, modes):
    """the sign rule: the largest-magnitude score of every mode is positive, ties (magnitudes within 1e-9 relative of the largest: what is a tie
    in exact arithmetic must stay one in floating point) to the lowest member index"""
    for m in range(scores.shape[1]):
        mag = np.abs(scores[:, m])
        i = int(np.nonzero(mag >= mag.max() * (1 - 1e-9))[0][0])
        if scores[i, m] < 0:
            scores[:, m] *= -1
            modes[m] *= -1
    return scores, modes


def pga_ref(a, y, n_modes, center=True, covariates=None):
    """a [B, k, N], y [k, N] with orthonormal rows -> dict with the fields of geometry.grassmann_pga's info (numpy float64) plus ``modes`` [M, k, N],
    ``logs`` and ``mean_tangent``; ``spectrum``: all eigenvalues of the tangent covariance"""
    logs, theta = logs_at(y, a)
    b, k, n = logs.shape
    flat = logs.reshape(b, -1)
    mean = flat.mean(axis=0)
    x = flat - mean if center else flat.copy()
    u, s, vt = np.linalg.svd(x, full_matrices=False)
    spectrum = s ** 2 / b
    m = n_modes
    modes = vt[:m].copy()
    scores = x @ modes.T
    scores, modes = fix_signs(scores, modes)
    total = float(np.sum(x * x) / b)
    out = {"logs": logs, "theta": theta, "tangent_gram": flat @ flat.T, "variance": spectrum[:m].copy(), "spectrum": spectrum, "total_variance": total,
           "explained": np.cumsum(spectrum[:m]) / total if total > 0 else np.zeros(m), "scores": scores,
           "residual": np.linalg.norm(x - scores @ modes, axis=1), "mean_tangent": mean.reshape(k, n), "mean_tangent_norm": float(np.linalg.norm(mean)),
           "modes": modes.reshape(m, k, n)}
    if covariates is not None:
        xs = np.asarray(covariates, np.float64).reshape(b, -1)
        design = np.concatenate([np.ones((b, 1)), xs], axis=1)
        coef, *_ = np.linalg.lstsq(design, flat, rcond=None)
        fit = design @ coef
        cen = flat - mean
        out["intercept"] = coef[0].reshape(k, n)
        out["slopes"] = coef[1:].reshape(-1, k, n)
        ss = float(np.sum(cen * cen))
        out["r2"] = float(np.sum((fit - mean) ** 2) / ss) if ss > 0 else 0.0
        out["slope_norm"] = np.linalg.norm(coef[1:], axis=1)
    return out


def operator_gap(p1, h1, p2, h2):
    """||op(p1, h1) - op(p2, h2)||_F / ||op(p2, h2)||_F for op = _grassmann_ref.tangent_operator, the N x N map p_i -> h_i (zero on the complement of span
    p): with g = (p p^T)^-1 p the operator is h^T g, and ||h1^T g1 - h2^T g2||_F^2 expands into traces of k x k Grams -- the same number without an
    N x N matrix.  The expansion cancels to 1e-8 relative in float64, two decades below the 1e-6 bar."""
    p1, h1, p2, h2 = (np.asarray(x, np.float64) for x in (p1, h1, p2, h2))
    g1, g2 = np.linalg.solve(p1 @ p1.T, p1), np.linalg.solve(p2 @ p2.T, p2)
    a = np.sum((h1 @ h1.T) * (g1 @ g1.T))
    b = np.sum((h2 @ h2.T) * (g2 @ g2.T))
    c = np.sum((h1 @ h2.T) * (g1 @ g2.T))
    return float(np.sqrt(max(a + b - 2 * c, 0.0) / b)) if b > 0 else float(np.sqrt(max(a, 0.0)))


def relative_gaps(spectrum, m):
    """(lambda_j - lambda_{j+1}) / lambda_j after each of the first m modes (a missing next eigenvalue counts as 0)"""
    s = np.concatenate([np.asarray(spectrum, np.float64), np.zeros(m + 1)])
    return np.array([(s[j] - s[j + 1]) / s[j] for j in range(m)])


# ------------------------------------------------------------------------------------------------------------ the k x k identity of the pair kernel
def tangent_gram_identity(a, y):
    """T [B, B] from k x k algebra only.  With Q_i orthonormal, M_i = Y Q_i^T, I - M_i M_i^T = V sin^2(theta) V^T, F_i = V theta / (sin cos) V^T,
    E_i = F_i M_i and K_i = F_i M_i M_i^T the tangent is L_i = E_i Q_i - K_i Y; since Y Y^T = I and Q_a Y^T = M_a^T,
    <L_a, L_b> = tr(E_a Ghat_ab E_b^T) - tr(K_a K_b), Ghat_ab = Q_a Q_b^T: each pair touches its own k x k block of the whitened Gram only."""
    qs = [F.orthonormal_rows(x) for x in np.asarray(a, np.float64)]
    es, ks = [], []
    for q in qs:
        m = y @ q.T
        lam, v = np.linalg.eigh(np.eye(len(y)) - m @ m.T)
        sn = np.sqrt(np.clip(lam, 0.0, 1.0))
        cs = np.linalg.norm(v.T @ m, axis=1)
        th = np.arctan2(sn, cs)
        f = np.where(sn > 0, th / np.where(sn > 0, sn * cs, 1.0), 1.0)
        fm = (v * f) @ v.T
        es.append(fm @ m)
        ks.append(fm @ m @ m.T)
    b = len(qs)
    t = np.zeros((b, b))
    for i in range(b):
        for j in range(b):
            t[i, j] = np.sum((es[i] @ (qs[i] @ qs[j].T)) * es[j]) - np.sum(ks[i] * ks[j])
    return t


# ------------------------------------------------------------------------------------------------------------ planted sets
def frobenius_orthonormal_tangents(rng, y, m):
    """m tangents at Y (rows orthogonal to the rows of Y), orthonormal under <A, B> = tr(A B^T)"""
    k, n = y.shape
    h = rng.standard_normal((m, k, n))
    h -= (h @ y.T) @ y
    q, _ = np.linalg.qr(h.reshape(m, -1).T)
    return q.T.reshape(m, k, n)


def mode_sds(m, first=0.5, ratio=1.8):
    """per-mode standard deviations spaced by `ratio` (>= 1.6): 0.5, 0.28, 0.15, ..."""
    return first / ratio ** np.arange(m)


def planted_set(rng, b, k, n, m, noise=0.0, covariate=None, cond=30.0):
    """(members [b, k, N] float32, Y0 [k, N], D [m, k, N], c [b, m]): members Exp_{Y0}(sum_m c_im D_m + noise) with c_im uniform of standard deviation
    mode_sds(m)[m] -- bounded, so the largest angle to Y0 stays below ||c_i||_2 + noise <= sqrt(3) ||sds||_2 < 1.1 rad -- rows remixed by a matrix of
    condition <= cond and scaled.  covariate [b]: c_i0 is made exactly linear in it, scaled to the planted standard deviation."""
    y0 = F.random_orthonormal(rng, k, n)
    d = frobenius_orthonormal_tangents(rng, y0, m)
    sds = mode_sds(m)
    c = sds * np.sqrt(3.0) * rng.uniform(-1.0, 1.0, (b, m))
    if covariate is not None:
        x = np.asarray(covariate, np.float64)
        c[:, 0] = sds[0] * np.sqrt(3.0) * (x - x.mean()) / np.abs(x - x.mean()).max()
    members = []
    for i in range(b):
        t = np.tensordot(c[i], d, axes=1)
        if noise > 0:
            e = rng.standard_normal((k, n))
            e -= (e @ y0.T) @ y0
            t = t + noise * e / np.linalg.norm(e)
        members.append(rng.uniform(0.5, 2.0) * F.mixing(rng, k, cond) @ F.exp_map(y0, t))
    return np.stack(members).astype(np.float32), y0, d, c
