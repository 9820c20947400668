"""References of the pullback geodesic (csrc/geodesic_chain.hip, dpb_geodesic_chain, PullbackUNet.pullback_geodesic).  Test infrastructure, not
imported by the product.

``cotangents_ref`` / ``update_ref``: numpy float64 restatements of dpb_geodesic_cotangents and dpb_geodesic_update as include/dpb.h states them (the
sums are numpy's, so they agree with the device's fixed chains to a few fp64 roundings, not bitwise -- exactly where every term is exact).
round32=False keeps everything in float64: the formulas alone, for the comparison with autograd.
``geodesic_ref``: the chain on a CPU net in the dtype asked for.  The gradient is torch.autograd's of the ENERGY ITSELF, E_h = 1/2 sum ||h_{i+1} -
h_i||^2 and E_x = 1/2 sum ||P_{i+1} - P_i||^2 -- never the formula J^T c, which is what the device computes and these references test.
``descent_ref``: the host driver of pullback_geodesic restated, with the relative margin of every decision it takes.
"""
import math

import numpy as np
import torch


def cotangents_ref(h, round32=True):
    """h [m + 2, D] float32 (float64 when not round32) -> (cot [m, D], seg [m + 1] f64, csq [m] f64)"""
    h = np.asarray(h, np.float32 if round32 else np.float64).astype(np.float64)
    with np.errstate(all="ignore"):
        cot = (2.0 * h[1:-1] - h[:-2]) - h[2:]
        if round32:
            cot = cot.astype(np.float32)
        d = h[1:] - h[:-1]
        return cot, (d * d).sum(1), (cot.astype(np.float64) ** 2).sum(1)


def update_ref(P, W, eta, lam=0.0, round32=True):
    """P [m + 2, N], W [m, N] float32 -> (P_out [m + 2, N], stats [m, 4] f64 = (sum W^2, sum g^2, sum (P_out - P)^2, flag), xseg [m + 1] f64).  eta and
    lam are the fp32 values the entry point takes.  A row whose W_i, P_i or neighbours hold a non-finite value: flag 1 and NaN in that row of P_out."""
    ft = np.float32 if round32 else np.float64
    P, W = np.asarray(P, ft), np.asarray(W, ft)
    eta, lam = (float(np.float32(eta)), float(np.float32(lam))) if round32 else (float(eta), float(lam))
    p, w = P.astype(np.float64), W.astype(np.float64)
    with np.errstate(all="ignore"):
        g = w + lam * ((2.0 * p[1:-1] - p[:-2]) - p[2:])
        out = P.copy()
        out[1:-1] = P[1:-1] if eta == 0.0 else (p[1:-1] - eta * g).astype(ft)
        dx = out[1:-1].astype(np.float64) - p[1:-1]
        bad = ~(np.isfinite(w).all(1) & np.isfinite(p[1:-1]).all(1) & np.isfinite(p[:-2]).all(1) & np.isfinite(p[2:]).all(1))
        out[1:-1][bad] = np.nan
        stats = np.stack([(w * w).sum(1), (g * g).sum(1), (dx * dx).sum(1), bad.astype(np.float64)], axis=1)
        d = p[1:] - p[:-1]
        return out, stats, (d * d).sum(1)


def get_hs(kind, tap, dtype, t, ctx=None):
    """one CPU get_h per point of a curve on the toy nets of tests/test_gpu_inv_jac_chain.py, parameters in `dtype`, every point at the timestep t,
    point i with row i of ctx [m + 2, L, D] (SD).  The dtype handling of that file's _get_hs."""
    import _adm_ref as A
    import test_gpu_inv_jac_chain as IJ
    cfg, p, _, _ = IJ._model(kind)
    p = {k: v.to(dtype) for k, v in p.items()}
    if kind == "sd":
        from oracle import unet_sd
        return [lambda a, b=b: unet_sd.forward(p, cfg, a, torch.tensor(t), ctx[b:b + 1].to(dtype), stop=tap) for b in range(ctx.shape[0])]
    if kind == "ddpm":
        from oracle import unet_ddpm
        emb = unet_ddpm.timestep_embedding

        def fwd(a):                                                  # the oracle's sinusoid is fp32 whatever the parameters: cast it for the float64 run
            unet_ddpm.timestep_embedding = lambda tt, d: emb(tt, d).to(dtype)
            try:
                return unet_ddpm.forward(p, cfg, a, torch.tensor(t), stop=tap)
            finally:
                unet_ddpm.timestep_embedding = emb
        return fwd
    return lambda a: A.get_h(p, cfg, a, t)


def _h_of(get_hs, P):
    """h [m + 2, D] of the curve P [m + 2, ...]: get_hs is one callable for every point, or one per point"""
    one = lambda i: (get_hs[i] if isinstance(get_hs, (list, tuple)) else get_hs)(P[i:i + 1]).reshape(1, -1)
    return torch.cat([one(i) for i in range(P.shape[0])])


def energies(get_hs, P):
    """(E_h, E_x, seg_h [m + 1], seg_x [m + 1]) as tensors of P's dtype, differentiable in P"""
    h = _h_of(get_hs, P)
    seg_h = ((h[1:] - h[:-1]) ** 2).sum(1)
    seg_x = ((P[1:] - P[:-1]) ** 2).flatten(1).sum(1)
    return 0.5 * seg_h.sum(), 0.5 * seg_x.sum(), seg_h, seg_x


def gradients(get_hs, P):
    """autograd of the energy itself at the curve P [m + 2, ...]: (dE_h/dP_i, dE_x/dP_i) for the interior rows [m, N], seg_h, seg_x, h"""
    Pv = P.detach().clone().requires_grad_(True)
    eh, ex, seg_h, seg_x = energies(get_hs, Pv)
    gh, = torch.autograd.grad(eh, Pv, retain_graph=True)
    gx, = torch.autograd.grad(ex, Pv)
    return gh[1:-1].flatten(1).detach(), gx[1:-1].flatten(1).detach(), seg_h.detach(), seg_x.detach()


def geodesic_ref(get_hs, P, eta, lam, iters, dtype=torch.float64, final_energy=True):
    """The chain on a CPU net: P [m + 2, C, H, W]; everything after the inputs in `dtype`; iteration j: g_i = dE/dP_i by autograd, P_i <- P_i - eta
    g_i for the interior rows.  Returns float64 tensors: curves [iters + 1, m + 2, ...], seg_h, seg_x [iters + 1, m + 1] (the last row NaN unless
    final_energy), stats [iters, m, 4] = (||dE_h/dP_i||^2, ||g_i||^2, ||P_out_i - P_i||^2, 0), csq [iters, m] = ||2 h_i - h_{i-1} - h_{i+1}||^2."""
    P = P.to(dtype)
    m = P.shape[0] - 2
    eta_t, lam_t = torch.tensor(float(eta), dtype=dtype), torch.tensor(float(lam), dtype=dtype)
    curves, sh, sx, stats, csq = [P], [], [], [], []
    for j in range(iters):
        gh, gx, seg_h, seg_x = gradients(get_hs, curves[-1])
        with torch.no_grad():
            h = _h_of(get_hs, curves[-1])
            c = 2 * h[1:-1] - h[:-2] - h[2:]
            g = gh + lam_t * gx
            new = curves[-1].clone()
            new[1:-1] = curves[-1][1:-1] - (eta_t * g).view_as(new[1:-1])
            dx = (new[1:-1] - curves[-1][1:-1]).flatten(1)
        curves.append(new); sh.append(seg_h); sx.append(seg_x); csq.append((c * c).sum(1))
        stats.append(torch.stack([(gh * gh).sum(1), (g * g).sum(1), (dx * dx).sum(1), torch.zeros(m, dtype=dtype)], dim=1))
    if final_energy:
        with torch.no_grad():
            _, _, seg_h, seg_x = energies(get_hs, curves[-1])
    else:
        seg_h = seg_x = torch.full((m + 1,), float("nan"), dtype=dtype)
    sh.append(seg_h); sx.append(seg_x)
    return {"curves": torch.stack(curves).double(), "seg_h": torch.stack(sh).double(), "seg_x": torch.stack(sx).double(),
            "stats": torch.stack(stats).double(), "csq": torch.stack(csq).double()}


def step_rule(r):
    """eta_0 = 1/4 sum ||c_i||^2 / sum ||g_i||^2 from the first iteration of a chain record"""
    return 0.25 * float(r["csq"][0].sum()) / float(r["stats"][0, :, 1].sum())


def curve_stats(seg_h, seg_x, lam):
    seg_h, seg_x = seg_h.double(), seg_x.double()
    eh, ex = 0.5 * float(seg_h.sum()), 0.5 * float(seg_x.sum())
    lh = float(seg_h.sqrt().sum())
    return {"energy": eh + lam * ex, "energy_h": eh, "energy_x": ex, "length_h": lh, "length_x": float(seg_x.sqrt().sum()),
            "uniformity": lh * lh / (seg_h.numel() * float(seg_h.sum()))}


def descent_ref(get_hs, P0, lam=0.0, step_size=None, max_iter=200, tol=1e-4, check_every=4, max_halvings=8, dtype=torch.float64):
    """The driver of PullbackUNet.pullback_geodesic restated on geodesic_ref.  Blocks of check_every iterations at one eta; a block whose end energy is
    not finite or above its start energy is discarded and eta halved (max_halvings in a row: stop, not converged); an accepted block with E_start -
    E_end <= tol E_start ends the descent, converged; max_iter bounds the iterations run, discarded ones included; step_size None: the step rule from
    a probe.  Returns (curve float64, info): info as the product's, and `margins`: for every block the relative distance |E_end - E_start| / E_start
    of its accept / reject decision and, for an accepted block, |(E_start - E_end) - tol E_start| / (tol E_start) of its stop decision."""
    E = lambda r, j: 0.5 * float(r["seg_h"][j].sum()) + lam * 0.5 * float(r["seg_x"][j].sum())
    curve = P0.to(dtype)
    eta = step_rule(geodesic_ref(get_hs, curve, 0.0, lam, 1, dtype, False)) if step_size is None else float(step_size)
    info = dict(halvings=0, decisions=[], margins=[], converged=False, rises=0, iterations=0, energy=[])
    attempted = row = 0
    last = None
    while attempted < max_iter:
        n = min(check_every, max_iter - attempted)
        r = geodesic_ref(get_hs, curve, eta, lam, n, dtype, True)
        attempted += n
        e0, e1 = E(r, 0), E(r, n)
        if not info["energy"]:
            info["energy"].append(e0)
            info["start"] = {k: curve_stats(r["seg_h"][0], r["seg_x"][0], lam)[k] for k in ("energy", "length_h", "uniformity")}
            last = (r["seg_h"][0], r["seg_x"][0], r["stats"][0])
        ok = math.isfinite(e1) and e1 <= e0
        info["decisions"].append(ok)
        info["margins"].append(abs(e1 - e0) / e0 if math.isfinite(e1) else float("inf"))
        if not ok:
            eta, row = eta / 2, row + 1
            info["halvings"] += 1
            if row >= max_halvings:
                break
            continue
        row = 0
        es = [E(r, j) for j in range(n + 1)]
        info["rises"] += sum(es[j + 1] > es[j] for j in range(n))
        curve, last = r["curves"][n].to(dtype), (r["seg_h"][n], r["seg_x"][n], r["stats"][n - 1])
        info["iterations"] += n
        info["energy"].append(e1)
        if tol > 0:
            info["margins"].append(abs((e0 - e1) - tol * e0) / (tol * e0))
        if e0 - e1 <= tol * e0:
            info["converged"] = True
            break
    info.update({k: v for k, v in curve_stats(last[0], last[1], lam).items() if k != "energy"})      # (energy: the list of the block boundaries)
    info["monotone"] = all(b <= a for a, b in zip(info["energy"], info["energy"][1:]))
    info.update(seg_h=last[0], seg_x=last[1], grad_norm=last[2][:, 1].sqrt(), step_size=eta, attempted=attempted)
    return curve.double(), info
