"""The cases of tests/test_gpu_jac_lstsq.py and tests/test_gpu_newton_h_chain.py, computed once on the CPU and shared: the side-8 toy nets of
tests/test_gpu_inv_jac_chain.py with per-sample timesteps and three rows, their dense float64 Jacobians, and the oracle's solves and chains in
float64 (the reference) and in float32 (what measures the bars).  Test infrastructure, not imported by the product."""
import functools

import numpy as np
import torch

import _cgls_ref as R
from test_gpu_inv_jac_chain import DIRS, SIGNS, TS, U_SEED, _get_hs, _model

CASES = [("ddpm", ("mid", 0)), ("ddpm", ("up", 1)), ("adm", ("mid", 0)), ("sd", ("mid", 0)), ("sd", ("down", 0))]
C_SEED = 34
REGIMES = {"fixed": dict(iters=8, tol=0.0), "converged": dict(iters=32, tol=1e-6)}
CHAIN = dict(steps=2, iters=8, tol=0.0, frac=0.25)            # the chain's target: a shift of frac * ||h0|| along its direction


@functools.lru_cache(maxsize=None)
def jacobians(kind, tap):
    """(J [3] float64 arrays [D, N] at the three samples and timesteps, the largest sigma_1^2 among them, h0 [3, D] float64)"""
    _, _, x, _ = _model(kind)
    g64 = _get_hs(kind, tap, torch.float64, TS)
    Js, h0 = [], []
    for b in range(x.shape[0]):
        xb = x[b:b + 1].double()
        J = torch.func.jacfwd(lambda a: g64[b](a).reshape(-1))(xb)
        Js.append(J.reshape(J.shape[0], -1).numpy())
        with torch.no_grad():
            h0.append(g64[b](xb).reshape(-1).numpy())
    s1 = max(float(np.linalg.norm(J, 2)) ** 2 for J in Js)
    return Js, s1, np.stack(h0)


def rhs(kind, tap):
    D = jacobians(kind, tap)[0][0].shape[0]
    return torch.randn(3, D, generator=torch.Generator().manual_seed(C_SEED))


def rel_rows(a, b):
    """the worst row of ||a_b - b_b|| / ||b_b||"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)).max())


@functools.lru_cache(maxsize=None)
def solve_bars(kind, tap, regime):
    """mu = 0.1 sigma_1^2; the float64 and the float32 oracle solves and the dense solution; d64 / d32: their distances (relative in ||delta||) from
    what the regime compares with -- the float64 restatement (fixed) or the dense solve (converged)"""
    _, _, x, _ = _model(kind)
    Js, s1, _ = jacobians(kind, tap)
    mu, kw = 0.1 * s1, REGIMES[regime]
    c = rhs(kind, tap).numpy()
    d64, h64 = R.net_solve_ref(_get_hs(kind, tap, torch.float64, TS), x, c, mu, 0.0, kw["tol"], kw["iters"], torch.float64)
    d32, h32 = R.net_solve_ref(_get_hs(kind, tap, torch.float32, TS), x, c, mu, 0.0, kw["tol"], kw["iters"], torch.float32)
    dense = np.stack([R.dense_solve(J, c[b].astype(np.float64), mu) for b, J in enumerate(Js)])
    want = d64 if regime == "fixed" else dense
    return dict(mu=mu, c=c, ref64=d64, hist64=h64, ref32=d32, hist32=h32, dense=dense, want=want, d32=rel_rows(d32, want), d64=rel_rows(d64, dense))


def chain_inputs(kind, tap):
    """(u [D, 2] Gaussian, scale [3]: a quarter of ||h0|| along the unit direction, mu)"""
    Js, s1, h0 = jacobians(kind, tap)
    u = torch.randn(h0.shape[1], 2, generator=torch.Generator().manual_seed(U_SEED))
    scale = [float(np.float32(CHAIN["frac"] * np.linalg.norm(h0[b]) / float(u[:, DIRS[b]].norm()))) for b in range(3)]
    return u, scale, 0.1 * s1


KEYS = ("states", "h_shift", "h_dist")


def chain_dist(a, b, sigma):
    """how far two chains are apart, absolute over the shift asked for (sigma_b ||c_b||, per chain)"""
    out = {}
    for k in KEYS:
        d = np.abs(np.asarray(a[k], np.float64) - np.asarray(b[k], np.float64)).reshape(3, -1).max(axis=1)
        out[k] = float((d / np.asarray(sigma)).max())
    return out


@functools.lru_cache(maxsize=None)
def chain_bars(kind, tap):
    """(ref64, d): the float64 chain and the float32 oracle's distance from it per key"""
    _, _, x, _ = _model(kind)
    u, scale, mu = chain_inputs(kind, tap)
    c = torch.stack([SIGNS[b] * u[:, DIRS[b]] for b in range(3)]).numpy()
    run = lambda dt: R.newton_chain_ref(_get_hs(kind, tap, dt, TS), x, c, scale, CHAIN["steps"], CHAIN["iters"], mu, 0.0, CHAIN["tol"], 0.0, dt)
    ref64, ref32 = run(torch.float64), run(torch.float32)
    sigma = [scale[b] * float(np.linalg.norm(c[b])) for b in range(3)]
    return ref64, chain_dist(ref32, ref64, sigma), sigma
