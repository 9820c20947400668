"""Numpy float64 reference of the weighted flag mean and the flag median (FlagIRLS; Mankovich, King, Peterson, Kirby, CVPR 2022), in the AMBIENT
space on purpose: every member is orthonormalised by QR, the rows sqrt(what_i) Q_i are stacked and go through one SVD per round -- none of the Gram /
coefficient algebra of csrc/flagmean.hip.  Same eps, tol and stop rule as geometry.flag_median.

Also the planted sets of the tests: a majority of members around one r-frame and outliers around another (or around random ones)."""
import numpy as np

import _flag_ref as R
from _frechet_ref import angles_to, max_angle, mixing, orthonormal_rows, random_orthonormal  # noqa: F401


def normalised(w, b):
    """the weights scaled to mean 1"""
    w = np.asarray(w, np.float64)
    return w * b / w.sum()


def weighted_flag_mean_ref(a, r=None, weights=None, qs=None):
    """a [B, k, N] -> (Y [r, N] float64, info): weight [r] and eigenvalues (sigma^2 / B of the stacked sqrt(what_i) Q_i, what of mean 1), theta
    [B, min(r, k)] descending (of EVERY member, weight 0 included), affinity [B] = ||Q_i Y^T||_F^2, member_weight [B] = what"""
    a = np.asarray(a, dtype=np.float64)
    b, k, _ = a.shape
    r = k if r is None else r
    qs = [orthonormal_rows(x) for x in a] if qs is None else qs
    what = np.ones(b) if weights is None else normalised(weights, b)
    _, s, vt = np.linalg.svd(np.concatenate([np.sqrt(w) * q for w, q in zip(what, qs)]), full_matrices=False)
    y = vt[:r]
    ev = s ** 2 / b
    theta = np.stack([angles_to(y, q) for q in qs])
    aff = np.array([np.sum((q @ y.T) ** 2) for q in qs])
    return y, {"weight": ev[:r], "eigenvalues": ev, "theta": theta, "affinity": aff, "member_weight": what}


def phi(d, eps):
    """the smoothed distance IRLS with the clamped weight 1 / max(d, eps) descends"""
    d = np.asarray(d, np.float64)
    return np.where(d >= eps, d, d * d / (2.0 * eps) + 0.5 * eps)


def flag_median_ref(a, r=None, eps=1e-5, max_rounds=50, tol=1e-9, weights=None):
    """a [B, k, N] -> (Y [r, N], info).  Round 0 is the (prior-weighted) flag mean; round t the weighted flag mean under p_i / max(d_i, eps) of round
    t - 1, scaled to mean 1; J = sum_i p_i phi(d_i); stop when J_prev - J <= tol J_prev or after max_rounds reweightings.  info: rounds, converged,
    objective, monotone, member_weight (of the last solve), distance, affinity, weight, eigenvalues, theta (of the last solve) and, per round,
    ``gaps`` (the relative gap after row r of that round's spectrum) and ``dmin`` (min_i d_i)."""
    a = np.asarray(a, dtype=np.float64)
    b, k, _ = a.shape
    r = k if r is None else r
    assert 1 <= r <= k
    qs = [orthonormal_rows(x) for x in a]
    p = np.ones(b) if weights is None else normalised(weights, b)
    what = p.copy()
    objective, gaps, dmin, converged = [], [], [], False
    while True:
        y, mi = weighted_flag_mean_ref(a, r, what, qs)
        d = np.sqrt(np.maximum(r - mi["affinity"], 0.0))
        objective.append(float(np.sum(p * phi(d, eps))))
        gaps.append(float(R.rel_gaps(mi["eigenvalues"])[r - 1]))
        dmin.append(float(d.min()))
        if len(objective) >= 2 and objective[-2] - objective[-1] <= tol * objective[-2]:
            converged = True
            break
        if len(objective) > max_rounds:
            break
        what = normalised(p / np.maximum(d, eps), b)
    objective = np.array(objective)
    info = dict(mi)
    info.update({"rounds": len(objective) - 1, "converged": converged, "objective": objective,
                 "monotone": bool(np.all(objective[1:] <= objective[:-1] * (1.0 + 1e-12))), "distance": d, "gaps": np.array(gaps),
                 "dmin": np.array(dmin)})
    return y, info


def planted(rng, b_in, b_out, k, n, r, noise=0.2, cond=10.0, out_shared=True):
    """(members [b_in + b_out, k, N] float32, frame [r, N]): b_in members hold frame + noise g / sqrt(N) (r rows), b_out members the same around a
    second r-frame (out_shared) or around a fresh random r-frame each; every member has k - r private Gaussian rows and its rows mixed by a matrix of
    condition cond.  The inliers come first."""
    frame = random_orthonormal(rng, r, n)
    other = random_orthonormal(rng, r, n)
    out = []
    for i in range(b_in + b_out):
        centre = frame if i < b_in else (other if out_shared else random_orthonormal(rng, r, n))
        rows = centre + noise * rng.standard_normal((r, n)) / np.sqrt(n)
        rows = np.concatenate([rows, rng.standard_normal((k - r, n)) / np.sqrt(n)])
        out.append(mixing(rng, k, cond) @ rows)
    return np.stack(out).astype(np.float32), frame


# the planted sets of the tests: (b_in, b_out, k, n, r), seed, out_shared
PLANTED = [((12, 8, 6, 200, 3), 0, True), ((24, 16, 32, 2050, 10), 0, True), ((5, 4, 8, 130, 4), 1, True), ((7, 4, 4, 67, 2), 1, False),
           ((2, 1, 64, 4099, 64), 0, False), ((3, 0, 2, 9, 1), 1, False)]
MIN_GAP, MIN_DIST = 0.05, 1e-3          # the conditions under which per-round and final-span claims are made


def qualifies(info):
    """every round shows a relative gap >= 0.05 after row r and every d_i >= 1e-3 (sqrt does not amplify the affinity's rounding)"""
    return bool(info["gaps"].min() >= MIN_GAP and info["dmin"].min() >= MIN_DIST)
