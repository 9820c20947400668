"""References of the least-squares inverse and the newton-h chain (csrc/cgls.hip, dpb_jac_lstsq, dpb_newton_h_chain).  Test infrastructure, not
imported by the product.

``init_ref`` / ``h_step_ref`` / ``x_step_ref``: numpy float64 restatements of dpb_cgls_init / _h_step / _x_step as include/dpb.h states them, R rows
at once.  ``store`` is the type the vectors delta, r, p are kept in: float32 restates the kernels (every element formed in float64 from the stored
operands and rounded once), float64 is the recurrence itself.  The sums are numpy's, so they agree with the device's fixed chains to a few fp64
roundings, not bitwise.  ``solve_ref`` runs the recurrence around two callables (q = J p, w = J^T r); ``dense_solve`` is (J^T J + mu I)^-1 J^T c.
``residual_ref`` / ``update_ref``: dpb_newton_residual and dpb_newton_update.  ``net_solve_ref`` / ``newton_chain_ref``: the solve and the chain on a
CPU net through oracle.pullback.jvp_step / vjp_step, in the dtype asked for.
"""
import numpy as np
import torch

GAMMA, GAMMA0, MU, RR, DD, FLAG, CC, ITERS = range(8)


class Rows:
    """delta, p [R, N] and r [R, D] in `store`, state [R, 8] float64"""

    def __init__(self, delta, r, p, state):
        self.delta, self.r, self.p, self.state = delta, r, p, state

    def copy(self):
        return Rows(self.delta.copy(), self.r.copy(), self.p.copy(), self.state.copy())

    def hist(self):
        return self.state[:, [GAMMA, RR, DD, FLAG]].copy()


def _sumsq(a):
    with np.errstate(all="ignore"):
        a = a.astype(np.float64)
        return (a * a).sum(axis=1)


def init_ref(c, w0, mu_abs=0.0, mu_rel=0.0, tol=0.0, store=np.float32):
    c = np.asarray(c, store); w0 = np.asarray(w0, store)
    R = c.shape[0]
    g0, cc = _sumsq(w0), _sumsq(c)
    S = Rows(np.zeros_like(w0), c.copy(), w0.copy(), np.zeros((R, 8)))
    for b in range(R):
        st = S.state[b]
        if not (np.isfinite(g0[b]) and np.isfinite(cc[b])):
            S.delta[b] = np.nan; S.r[b] = np.nan; S.p[b] = np.nan
            st[:] = np.nan; st[FLAG] = 3.0; st[ITERS] = 0.0
            continue
        mu, flag = mu_abs, 0
        if g0[b] <= tol * tol * g0[b]:
            flag = 1
        elif not cc[b] > 0.0:
            flag = 2
        else:
            mu = mu_abs + mu_rel * g0[b] / cc[b]
            flag = 0 if np.isfinite(mu) else 2
        st[:] = (g0[b], g0[b], mu, cc[b], 0.0, flag, cc[b], 0.0)
    return S, S.hist()


def h_step_ref(S, q):
    """in place on S; returns the history row"""
    store = S.delta.dtype
    q = np.asarray(q, store)
    pp, qq = _sumsq(S.p), _sumsq(q)
    for b in range(S.state.shape[0]):
        st = S.state[b]
        if st[FLAG] != 0.0:
            continue
        if not (np.isfinite(pp[b]) and np.isfinite(qq[b])):
            S.delta[b] = np.nan; S.r[b] = np.nan; S.p[b] = np.nan
            st[[GAMMA, RR, DD]] = np.nan; st[FLAG] = 3.0
            continue
        den = qq[b] + st[MU] * pp[b]
        if not (den > 0.0 and np.isfinite(den)):
            st[FLAG] = 2.0
            continue
        alpha = st[GAMMA] / den
        S.delta[b] = (S.delta[b].astype(np.float64) + alpha * S.p[b].astype(np.float64)).astype(store)
        S.r[b] = (S.r[b].astype(np.float64) + (-alpha) * q[b].astype(np.float64)).astype(store)
        st[DD] = _sumsq(S.delta[b:b + 1])[0]; st[RR] = _sumsq(S.r[b:b + 1])[0]
    return S.hist()


def x_step_ref(S, w, tol=0.0):
    store = S.delta.dtype
    w = np.asarray(w, store)
    for b in range(S.state.shape[0]):
        st = S.state[b]
        if st[FLAG] != 0.0:
            continue
        with np.errstate(all="ignore"):
            s = w[b].astype(np.float64) - st[MU] * S.delta[b].astype(np.float64)
            g1 = (s * s).sum()
        st[ITERS] += 1.0
        if not np.isfinite(g1):
            S.delta[b] = np.nan; S.r[b] = np.nan; S.p[b] = np.nan
            st[[GAMMA, RR, DD]] = np.nan; st[FLAG] = 3.0
            continue
        beta = g1 / st[GAMMA]
        S.p[b] = (s + beta * S.p[b].astype(np.float64)).astype(store)
        st[GAMMA] = g1
        if g1 <= tol * tol * st[GAMMA0]:
            st[FLAG] = 1.0
    return S.hist()


def solve_ref(matvec, rmatvec, c, mu_abs=0.0, mu_rel=0.0, tol=0.0, iters=8, store=np.float64):
    """matvec: p [R, N] -> J p [R, D]; rmatvec: r [R, D] -> J^T r [R, N], both per row.  Returns (Rows, hist [iters + 1, R, 4])."""
    c = np.asarray(c, store)
    S, h0 = init_ref(c, np.asarray(rmatvec(c), store), mu_abs, mu_rel, tol, store)
    hist = [h0]
    for _ in range(iters):
        if (S.state[:, FLAG] != 0).all():                      # every row is frozen: the remaining rounds hand everything through
            hist.append(S.hist())
            continue
        h_step_ref(S, np.asarray(matvec(S.p), store))
        hist.append(x_step_ref(S, np.asarray(rmatvec(S.r), store), tol))
    return S, np.stack(hist)


def dense_solve(J, c, mu):
    """(J^T J + mu I)^-1 J^T c in float64; mu = 0 on a rank-deficient J: the minimum-norm solution J^+ c"""
    J = np.asarray(J, np.float64); c = np.asarray(c, np.float64)
    if mu == 0.0:
        return np.linalg.pinv(J) @ c
    return np.linalg.solve(J.T @ J + mu * np.eye(J.shape[1]), J.T @ c)


def residual_ref(h0, h, u, dirs, signs, scale, frac):
    h0 = np.asarray(h0, np.float32).astype(np.float64); h = np.asarray(h, np.float32).astype(np.float64)
    u = np.asarray(u, np.float32).astype(np.float64)
    out = np.empty(h0.shape, np.float32)
    for b in range(h0.shape[0]):
        f = float(frac) * float(np.float32(scale[b]))
        out[b] = ((h0[b] + f * (float(np.float32(signs[b])) * u[int(dirs[b])])) - h[b]).astype(np.float32)
    return out


def update_ref(x, delta, state, radius=0.0):
    """(x_out f32, step_stats f64 [n, 4])"""
    x = np.asarray(x, np.float32); delta = np.asarray(delta, np.float32)
    out = np.empty_like(x); stats = np.empty((x.shape[0], 4))
    for b in range(x.shape[0]):
        dd = state[b, DD]
        kappa = radius / np.sqrt(dd) if radius > 0.0 and dd > radius * radius else 1.0
        with np.errstate(all="ignore"):
            out[b] = (x[b].astype(np.float64) + kappa * delta[b].astype(np.float64)).astype(np.float32)
        stats[b] = (state[b, CC], dd, kappa if dd == dd else np.nan, state[b, FLAG])
    return out, stats


# ---- on a CPU net
def _passes(get_hs, xs, dtype):
    """per-row tangent and adjoint passes at the states xs [n, C, H, W] (row b through get_hs[b]) as numpy callables"""
    from oracle.pullback import jvp_step, vjp_step
    n = xs.shape[0]
    shapes = []
    with torch.no_grad():
        for b in range(n):
            shapes.append(get_hs[b](xs[b:b + 1].to(dtype)).shape)

    def matvec(p):
        out = []
        for b in range(n):
            v = torch.as_tensor(np.asarray(p[b], np.float64)).to(dtype).reshape(xs[b:b + 1].shape)
            out.append(jvp_step(get_hs[b], xs[b:b + 1].to(dtype), v, 1, 1, "zt").reshape(-1).double().numpy())
        return np.stack(out)

    def rmatvec(r):
        out = []
        for b in range(n):
            u = torch.as_tensor(np.asarray(r[b], np.float64)).to(dtype).reshape(shapes[b])
            out.append(vjp_step(get_hs[b], xs[b:b + 1].to(dtype), u).reshape(-1).double().numpy())
        return np.stack(out)

    return matvec, rmatvec


def _store(dtype):
    return np.float64 if dtype == torch.float64 else np.float32


def net_solve_ref(get_hs, xs, c, mu_abs, mu_rel, tol, iters, dtype=torch.float64):
    """the solve at n states, one right-hand side each, everything in `dtype`.  c [n, D].  Returns (delta [n, N] f64, hist [iters + 1, n, 4])"""
    matvec, rmatvec = _passes(get_hs, xs, dtype)
    S, hist = solve_ref(matvec, rmatvec, np.asarray(c, np.float64), mu_abs, mu_rel, tol, iters, _store(dtype))
    return S.delta.astype(np.float64), hist


def newton_chain_ref(get_hs, x, c, scale, steps, iters, mu_abs, mu_rel, tol, radius=0.0, dtype=torch.float64):
    """The chain of dpb_newton_h_chain on a CPU net, everything in `dtype`.  x [n, C, H, W]; c [n, D]: chain b's direction sign * u[dir]; scale: n
    floats.  Returns a dict of float64 arrays: states [n, steps + 1, N], h_shift / h_dist [n, steps + 1], delta_norm / clip [n, steps]."""
    n = x.shape[0]
    store = _store(dtype)
    cur = x.to(dtype)
    c64 = np.asarray(c, np.float64)
    chat = c64 / np.linalg.norm(c64, axis=1, keepdims=True)
    states, hs, hd, dn, clip = [cur.reshape(n, -1).double().numpy()], [], [], [], []
    h0 = None
    for j in range(steps + 1):
        with torch.no_grad():
            h = np.stack([get_hs[b](cur[b:b + 1]).reshape(-1).double().numpy() for b in range(n)]).astype(store)
        h0 = h if h0 is None else h0
        d = h.astype(np.float64) - h0.astype(np.float64)
        hs.append((d * chat).sum(axis=1)); hd.append(np.linalg.norm(d, axis=1))
        if j == steps:
            break
        f = (j + 1) / steps
        res = ((h0.astype(np.float64) + f * np.asarray(scale, np.float64)[:, None] * c64.astype(store).astype(np.float64)) - h.astype(np.float64)).astype(store)
        matvec, rmatvec = _passes(get_hs, cur, dtype)
        S, _ = solve_ref(matvec, rmatvec, res, mu_abs, mu_rel, tol, iters, store)
        dd = S.state[:, DD]
        kappa = np.where((radius > 0.0) & (dd > radius * radius), radius / np.sqrt(np.maximum(dd, 1e-300)), 1.0)
        nxt = (cur.reshape(n, -1).double().numpy() + kappa[:, None] * S.delta.astype(np.float64)).astype(store)
        dn.append(np.sqrt(dd)); clip.append(kappa)
        cur = torch.as_tensor(nxt).to(dtype).reshape(x.shape)
        states.append(nxt.astype(np.float64))
    return {"states": np.stack(states, axis=1), "h_shift": np.stack(hs, axis=1), "h_dist": np.stack(hd, axis=1),
            "delta_norm": np.stack(dn, axis=1), "clip": np.stack(clip, axis=1)}
