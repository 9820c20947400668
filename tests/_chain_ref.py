"""References of the parallel-h edit chain (csrc/chain.hip, dpb_inv_jac_chain).  Test infrastructure, not imported by the product.

``direction_step_ref`` / ``shift_stats_ref``: numpy float64 restatements of dpb_direction_step and dpb_shift_stats as include/dpb.h states them
(the sums are numpy's, so they agree with the device's fixed chains to a few fp64 roundings, not bitwise).
``chain_ref``: the chain itself on a CPU net -- v = -J^T c / ||J^T c|| through oracle.pullback.vjp_step (autograd), torch's own std / where for
the SEGA rule, in the dtype asked for (float64: the reference; float32: what measures the bars of tests/test_gpu_inv_jac_chain.py).
"""
import numpy as np
import torch


def direction_step_ref(W, x, step, sega_sigma=0.0):
    """W, x: float32 arrays [n, N]; step: n floats.  Returns (x_out f32, vk f32, stats f64 [n, 4], margin f64 [n, N]): margin is the relative
    distance | |v| - thr | / thr of every element from the SEGA threshold (inf when the rule is off for the row)."""
    W = np.asarray(W, dtype=np.float32); x = np.asarray(x, dtype=np.float32)
    n, N = W.shape
    step = np.broadcast_to(np.asarray(step, dtype=np.float32), (n,)).astype(np.float64)
    x_out = np.empty((n, N), np.float32); vk = np.empty((n, N), np.float32)
    stats = np.zeros((n, 4), np.float64); margin = np.full((n, N), np.inf)
    for b in range(n):
        w = W[b].astype(np.float64)
        with np.errstate(all="ignore"):
            S1, S2 = w.sum(), (w * w).sum()
        stats[b, 0] = S2
        if not (S2 > 0 and np.isfinite(S2)):
            stats[b, 3] = 1.0
            x_out[b] = np.nan; vk[b] = np.nan
            continue
        v = (-w / np.sqrt(S2)).astype(np.float32)
        kept = N
        if sega_sigma > 0 and N >= 2:
            std = np.sqrt(max(0.0, 1.0 - S1 * S1 / (N * S2)) / (N - 1))
            thr = float(sega_sigma) * std
            a = np.abs(v.astype(np.float64))
            cut = a < thr
            margin[b] = np.abs(a - thr) / thr if thr > 0 else np.inf
            v = np.where(cut, np.float32(0), v)
            kept = int(N - cut.sum())
            stats[b, 1] = std
        stats[b, 2] = kept
        vk[b] = v
        x_out[b] = (x[b].astype(np.float64) + step[b] * v.astype(np.float64)).astype(np.float32)
    return x_out, vk, stats, margin


def shift_stats_ref(h, h0, u, dirs, signs):
    """float64 [n, 2]: (<h - h0, c> / ||c||, ||h - h0||^2), c = signs[b] * u[dirs[b]]; h, h0 [n, D], u [nu, D] float32 arrays"""
    h = np.asarray(h, np.float32).astype(np.float64); h0 = np.asarray(h0, np.float32).astype(np.float64)
    u = np.asarray(u, np.float32).astype(np.float64)
    out = np.empty((h.shape[0], 2))
    for b in range(h.shape[0]):
        c = float(np.float32(signs[b])) * u[int(dirs[b])]
        d = h[b] - h0[b]
        out[b] = ((d * c).sum() / np.sqrt((c * c).sum()), (d * d).sum())
    return out


def chain_ref(get_hs, x, c, steps, step, sega_sigma=None, dtype=torch.float64):
    """The chain on a CPU net.  get_hs: one callable per chain, x_b [1, C, H, W] -> h [1, ...] in `dtype` (its parameters are in that dtype);
    x [n, C, H, W]; c [n, D]: chain b's cotangent sign * u[dir] (held fixed); step: n floats.  Everything after the inputs in `dtype`: the adjoint
    through oracle.pullback.vjp_step, v = -W / ||W||, torch's std / where for the SEGA rule (edit.py:1212-1214), x + step * v.  Returns a dict of
    float64 tensors: states [n, steps + 1, ...], vk [n, steps, N], norm / sega_std / sega_kept / sega_margin [n, steps] (the margin: the least relative distance of an element of v
    from the rule's threshold, inf when the rule is off), h_shift / h_dist [n, steps + 1]."""
    from oracle.pullback import vjp_step
    n = x.shape[0]
    out = dict(states=[], vk=[], norm=[], sega_std=[], sega_kept=[], sega_margin=[], h_shift=[], h_dist=[])
    for b in range(n):
        xb = x[b:b + 1].to(dtype)
        cb = c[b].to(dtype)
        chat = cb / cb.norm()
        states, vks, norms, stds, kepts, margins, hs, hd = [xb], [], [], [], [], [], [], []
        h0 = None
        for j in range(steps + 1):
            with torch.no_grad():
                h = get_hs[b](states[-1])
            h0 = h if h0 is None else h0
            d = (h - h0).reshape(-1)
            hs.append(float(d @ chat)); hd.append(float(d.norm()))
            if j == steps:
                break
            W = vjp_step(get_hs[b], states[-1], cb.reshape(h.shape)).reshape(-1)
            v = -W / W.norm()
            std, kept, margin = 0.0, v.numel(), float("inf")
            if sega_sigma is not None and sega_sigma > 0:
                sd = v.std()
                margin = float(((v.abs() - sega_sigma * sd).abs() / (sega_sigma * sd)).min())
                v = torch.where(v.abs() < sega_sigma * sd, torch.zeros_like(v), v)
                std, kept = float(sd), int((v != 0).sum())
            norms.append(float(W.norm())); stds.append(std); kepts.append(kept); margins.append(margin); vks.append(v)
            states.append(states[-1] + torch.tensor(float(step[b]), dtype=dtype) * v.view_as(xb))
        out["states"].append(torch.cat(states).double()); out["vk"].append(torch.stack(vks).double())
        for k, v_ in (("norm", norms), ("sega_std", stds), ("sega_kept", kepts), ("sega_margin", margins), ("h_shift", hs), ("h_dist", hd)):
            out[k].append(torch.tensor(v_, dtype=torch.float64))
    return {k: torch.stack(v) for k, v in out.items()}
