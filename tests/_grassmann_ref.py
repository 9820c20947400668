"""Numpy float64 TEXTBOOK restatement of the Grassmann geodesic, log and exp maps (Edelman, Arias & Smith 1998, section 2.5), in the ambient space on
purpose -- none of the Gram / whitening / Jacobi algebra of csrc/geodesic.hip: both bases are orthonormalised by QR, the tangent is
Delta = (I - Y0 Y0^T) Y1 (Y0^T Y1)^-1 = U tan(Theta) V^T (thin SVD), the geodesic Y0 V cos(t Theta) V^T + U sin(t Theta) V^T, the log map the N x N
operator U Theta V^T Y0^T.  The textbook works with COLUMNS (N x k); the functions here take and return ROWS ([k, N]) like geometry.py.

Also the planted inputs that tests/test_grassmann_host.py holds this file to and tests/test_gpu_grassmann.py runs on the GPU."""
import numpy as np
from scipy.linalg import subspace_angles

HALF_PI = np.pi / 2


def _qr_cols(a):
    """a [k, N] rows -> (Y [N, k] orthonormal columns, R [k, k]) with a^T = Y R"""
    return np.linalg.qr(np.asarray(a, dtype=np.float64).T)


def tangent(a, b):
    """(Y0, U, theta, Vt): Delta = U tan(theta) Vt, theta descending (the SVD's order of tan theta)"""
    y0, _ = _qr_cols(a)
    y1, _ = _qr_cols(b)
    m = y0.T @ y1
    delta = (y1 - y0 @ m) @ np.linalg.inv(m)
    u, s, vt = np.linalg.svd(delta, full_matrices=False)
    return y0, u, np.arctan(s), vt


def geodesic(a, b, ts):
    """[T, k, N]: a basis (rows) of the point at every t of the geodesic from span a (t = 0) to span b (t = 1)"""
    y0, u, th, vt = tangent(a, b)
    out = []
    for t in np.atleast_1d(ts):
        y = y0 @ vt.T @ np.diag(np.cos(t * th)) @ vt + u @ np.diag(np.sin(t * th)) @ vt
        out.append(y.T)
    return np.stack(out)


def log_operator(a, b):
    """the log map at span a of span b as the N x N operator U Theta V^T Y0^T: it takes a vector of span a to its image under the tangent"""
    y0, u, th, vt = tangent(a, b)
    return u @ np.diag(th) @ vt @ y0.T


def tangent_operator(p, h):
    """the N x N operator of the tangent given as (P, H) rows: p_i -> h_i, zero on the complement of span P"""
    p, h = np.asarray(p, np.float64), np.asarray(h, np.float64)
    return h.T @ np.linalg.solve(p @ p.T, p)


def exp_map(p, h, ts):
    """([T, k, N], sigma [k] descending): the geodesic shot from span p along the tangent p_i -> (h_i's component orthogonal to span p)"""
    q, r = _qr_cols(p)
    g = np.asarray(h, dtype=np.float64).T @ np.linalg.inv(r)       # the images of the orthonormal columns of Q: p^T = Q R, so Q = p^T R^-1
    g = g - q @ (q.T @ g)                                          # horizontal projection
    u, s, vt = np.linalg.svd(g, full_matrices=False)
    out = []
    for t in np.atleast_1d(ts):
        y = q @ vt.T @ np.diag(np.cos(t * s)) @ vt + u @ np.diag(np.sin(t * s)) @ vt
        out.append(y.T)
    return np.stack(out), s


def angles_to(y, q):
    """principal angles between the row spans of y and q, descending (scipy, float64), measured in an orthonormal basis of their joint span (the R
    factor of one QR: an isometry)"""
    y, q = np.asarray(y, np.float64), np.asarray(q, np.float64)
    r = np.linalg.qr(np.concatenate([y, q]).T, mode="r")
    return subspace_angles(r[:, :len(y)], r[:, len(y):])


def max_angle(y0, y1):
    return float(angles_to(y0, y1)[0])


# ---------------------------------------------------------------------------------------------------------------- planted inputs
def angle_set(name, k, rng):
    """the angle families of the tests, k angles each"""
    if name == "tiny":
        return np.full(k, 1e-6)
    if name == "mixed":
        base = np.array([0.0, 1e-6, 1e-4, 1e-2, 0.3, 1.0, HALF_PI - 1e-3])
        return base[(np.arange(k) * 3) % len(base)] if k < len(base) else np.resize(base, k)
    if name == "spread":
        return np.linspace(0.0, HALF_PI - 1e-3, k) if k > 1 else np.array([HALF_PI - 1e-3])
    if name == "random":
        return rng.uniform(0.0, 1.5, k)
    raise ValueError(name)


def planted_pair(rng, k, n, theta):
    """(a, b) float64 [k, N] with orthonormal rows and principal angles theta: a_i = e_i, b_i = cos e_i + sin f_i over a random orthonormal 2k-frame"""
    assert n >= 2 * k
    f = np.linalg.qr(rng.standard_normal((n, 2 * k)))[0].T
    e, g = f[:k], f[k:]
    return e.copy(), np.cos(theta)[:, None] * e + np.sin(theta)[:, None] * g


def scale_rows(rng, x):
    """rows scaled by logspace(0, 2) in a random order"""
    return rng.permutation(np.logspace(0, 2, len(x)))[:, None] * x


def mix_rows(rng, x, cond=10.0):
    """rows mixed by a random matrix of condition number cond (1 for k = 1)"""
    k = len(x)
    u = np.linalg.qr(rng.standard_normal((k, k)))[0]
    v = np.linalg.qr(rng.standard_normal((k, k)))[0]
    return (u * np.logspace(0, np.log10(cond), k)) @ v.T @ x


def family(rng, k, n, name, variant):
    """one fp32 pair of the tests: angle set `name`, variant 0 orthonormal rows, 1 rows scaled, 2 rows mixed (condition 10)"""
    a, b = planted_pair(rng, k, n, angle_set(name, k, rng))
    if variant == 1:
        a, b = scale_rows(rng, a), scale_rows(rng, b)
    elif variant == 2:
        a, b = mix_rows(rng, a), mix_rows(rng, b)
    return a.astype(np.float32), b.astype(np.float32)


def random_pair(k, n, bar=HALF_PI - 1e-3):
    """intersecting spans (2k > N): random rows, the first seed whose largest principal angle is below bar; chosen on the CPU"""
    for seed in range(1000):
        rng = np.random.default_rng(7000 + 131 * k + n + 1009 * seed)
        a = rng.standard_normal((k, n)).astype(np.float32)
        b = rng.standard_normal((k, n)).astype(np.float32)
        if max_angle(a, b) < bar:
            return a, b
    raise RuntimeError(f"no seed gives a largest angle below {bar} for k = {k}, N = {n}")
