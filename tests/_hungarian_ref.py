"""The Hungarian-matched mean of directions restated in numpy float64 with scipy.optimize.linear_sum_assignment ("Hungarian mean"):
the yardstick of geometry.hungarian_mean.  a [B, k, N]; xhat: the rows scaled to unit length in float64.

  anchor Y = xhat[init] (or a given [k, N] array, scaled to unit rows)
  sweep:   c_b = Y xhat_b^T;  d = 1 / max(|c|, 2^-40) ('1/cosine') or 1 - |c| ('cosine');  pi_b = argmin_pi sum_i d[i, pi(i)];
           sigma_b(i) = -1 if c_b[i, pi_b(i)] < 0 else +1;  Y_i <- normalise(sum_b sigma_b(i) xhat_{b, pi_b(i)}), rounded to float32 ONCE --
           the next sweep's anchor is that float32 array (scaled to unit rows again in float64)
  stop when no pi_b and no sigma_b changed from the previous sweep (converged) or after max_sweeps.
"""
import itertools

import numpy as np
from scipy.optimize import linear_sum_assignment

MIN_COS = 2.0 ** -40
DISTANCES = ("1/cosine", "cosine")


def unit_rows(x):
    x = np.asarray(x, dtype=np.float64)
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def cost_matrix(c, distance):
    c = np.abs(c)
    if distance == "1/cosine":
        return 1.0 / np.maximum(c, MIN_COS)
    if distance == "cosine":
        return 1.0 - c
    raise ValueError(distance)


def overlaps(xh, y):
    """c [B, k, k]: c[b, i, j] = <y_i, xhat_{b, j}>"""
    return np.einsum("in,bjn->bij", unit_rows(y), xh)


def assign(d):
    """scipy's optimum of one matrix: (col_of_row, total)"""
    r, c = linear_sum_assignment(d)
    assert (r == np.arange(len(d))).all()
    return c.astype(np.int32), float(d[r, c].sum())


def brute_force(d):
    """the optimal total by enumeration of all k! assignments (k <= 6)"""
    k = len(d)
    return min(sum(d[i, p[i]] for i in range(k)) for p in itertools.permutations(range(k)))


def mean_with(xh, perm, sign):
    """Y [k, N] float32 of given assignments: normalise(sum_b sign[b, i] xhat[b, perm[b, i]]), b in index order"""
    s = np.zeros(xh.shape[1:], dtype=np.float64)
    for b in range(xh.shape[0]):
        s += sign[b][:, None] * xh[b][perm[b]]
    return (s / np.linalg.norm(s, axis=1, keepdims=True)).astype(np.float32), s


def mean_with_f64(xh, perm, sign):
    """the same before the rounding to float32"""
    s = mean_with(xh, perm, sign)[1]
    return s / np.linalg.norm(s, axis=1, keepdims=True)


def sweep(xh, y, distance):
    """one sweep against the anchor y: perm, sign [B, k] int32, total [B], the cost matrices [B, k, k]"""
    c = overlaps(xh, y)
    d = cost_matrix(c, distance)
    b, k, _ = c.shape
    perm = np.zeros((b, k), dtype=np.int32)
    sign = np.zeros((b, k), dtype=np.int32)
    total = np.zeros(b)
    for i in range(b):
        perm[i], total[i] = assign(d[i])
        sign[i] = np.where(c[i][np.arange(k), perm[i]] < 0, -1, 1)
    return perm, sign, total, d


def objective(xh, y, perm):
    """sum_b sum_i |<y_i, xhat_{b, perm[b, i]}>|: what a 'cosine' sweep cannot decrease"""
    c = overlaps(xh, y)
    k = c.shape[1]
    return float(sum(np.abs(c[b][np.arange(k), perm[b]]).sum() for b in range(len(c))))


def hungarian_mean_ref(a, init=0, distance="1/cosine", max_sweeps=20, anchor=None):
    """Y [k, N] float32 and info: perm, sign, cost [sweeps, B], sweeps, converged, changed (per sweep), weight [k], objective (per sweep: the 'cosine'
    objective of the sweep's anchor under the sweep's assignment), Y64 (the last mean before its rounding)"""
    xh = unit_rows(a)
    b, k, _ = xh.shape
    y = xh[init] if anchor is None else np.asarray(anchor, dtype=np.float64)
    perm, sign = np.full((b, k), -1, dtype=np.int32), np.zeros((b, k), dtype=np.int32)
    costs, changed, obj, converged = [], [], [], False
    for _ in range(max_sweeps):
        p, s, total, _ = sweep(xh, y, distance)
        changed.append(int(((p != perm) | (s != sign)).sum()))
        perm, sign = p, s
        costs.append(total)
        obj.append(objective(xh, y, perm))
        y = mean_with(xh, perm, sign)[0]
        if changed[-1] == 0:
            converged = True
            break
    c = overlaps(xh, y)
    weight = np.mean([np.abs(c[i][np.arange(k), perm[i]]) for i in range(b)], axis=0)
    return y, dict(perm=perm, sign=sign, cost=np.stack(costs), sweeps=len(costs), converged=converged, changed=changed, weight=weight, objective=obj,
                   Y64=mean_with_f64(xh, perm, sign))


def planted_set(rng, b, k, n, sigma):
    """Members of one planted frame: y [k, N] orthonormal; member m holds, at row p_m[i], s_m[i] * scale * normalise(y_i + sigma g / sqrt(N)) with g
    standard normal, p_m a random permutation, s_m random signs and scale in [0.5, 2].  Returns a [B, k, N] float32, y, and the assignment a matching
    against member 0 must find: perm [B, k] (perm[m, i] = the row of member m that holds the direction of row i of member 0) and sign [B, k]."""
    y = np.linalg.qr(rng.standard_normal((n, k)))[0].T
    a = np.zeros((b, k, n))
    pos = np.zeros((b, k), dtype=np.int64)
    sgn = np.zeros((b, k), dtype=np.int64)
    for m in range(b):
        rows = unit_rows(y + sigma * rng.standard_normal((k, n)) / np.sqrt(n))
        pos[m] = rng.permutation(k)
        sgn[m] = rng.choice([-1, 1], size=k)
        a[m][pos[m]] = sgn[m][:, None] * rows * rng.uniform(0.5, 2.0, size=(k, 1))
    inv0 = np.argsort(pos[0])                                  # the direction held by row i of member 0
    perm = np.stack([pos[m][inv0] for m in range(b)]).astype(np.int32)
    sign = np.stack([sgn[m][inv0] * sgn[0][inv0] for m in range(b)]).astype(np.int32)
    return a.astype(np.float32), y, perm, sign


def gaussian_set(rng, b, k, n):
    return rng.standard_normal((b, k, n)).astype(np.float32)
