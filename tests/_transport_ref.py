"""Float64 restatement of dpb_transport_directions (csrc/transport.hip) and the crafted inputs of its tests.

    c[d][p][q] = <uhat_dst[d][q], uhat_src[pcs[p]]>,   w[d][p] = sum_q c[d][p][q] vhat_dst[d][q],   vk = w / ||w||_2,   coef_norm = ||c[d][p]||_2

with uhat / vhat the rows scaled to unit length -- the reference's arithmetic (src/modules/edit.py:824-828, :847-851, :890-891) in float64 on the same
fp32 inputs.  The bars of the GPU tests are derived from the number formats, not from what the kernel gives:
  coef, coef_norm   4 * 2^-24 absolute: the values are formed in fp64 and are <= 1 in magnitude for unit rows, so only the fp32 store rounds
  vk, per element   (k + 4) * 2^-24 * sum_q |c_q| |vhat_q[n]| / ||w||  +  2^-24 |ref[n]|: the fp32 dot-product bound for k terms plus the roundings of c,
                    of the row scale and of the final scale
  ||vk||_2          within 4 * 2^-24 of 1, in fp64
"""
import numpy as np
import torch

EPS = 2.0 ** -24
BAR_COEF = 4 * EPS
BAR_NORM = 4 * EPS


def ref_transport(u_src, u_dst, vT_dst, pcs=None):
    """fp64.  u_src [k, N_h], u_dst [D, k, N_h], vT_dst [D, k, N_x] (rows).  Returns vk [D, P, N_x], coef [D, P, k], coef_norm [D, P] and
    absw [D, P, N_x] = sum_q |c_q| |vhat_q[n]| / ||w|| (what the element-wise bar of vk scales with)."""
    u_src, u_dst, vT_dst = (torch.as_tensor(a).double() for a in (u_src, u_dst, vT_dst))
    if u_dst.dim() == 2:
        u_dst, vT_dst = u_dst[None], vT_dst[None]
    pcs = list(range(u_src.shape[0])) if pcs is None else list(pcs)
    us = u_src / u_src.norm(dim=1, keepdim=True)
    ud = u_dst / u_dst.norm(dim=2, keepdim=True)
    vd = vT_dst / vT_dst.norm(dim=2, keepdim=True)
    coef = torch.einsum("dqn,pn->dpq", ud, us[pcs])
    w = torch.einsum("dpq,dqn->dpn", coef, vd)
    wn = w.norm(dim=2, keepdim=True)
    absw = torch.einsum("dpq,dqn->dpn", coef.abs(), vd.abs()) / wn
    return w / wn, coef, coef.norm(dim=2), absw


def rows(rng, k, n):
    """k unit rows of length n: orthonormal when they fit (k <= n), else independent Gaussian directions"""
    a = rng.standard_normal((n, k)) if k <= n else None
    if a is not None:
        return np.linalg.qr(a)[0].T.copy()
    a = rng.standard_normal((k, n))
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def crafted(kind, k, nh, nx, D, seed=0):
    """fp32 (u_src [k, nh], u_dst [D, k, nh], vT_dst [D, k, nx]).  kind 'orthonormal': unit rows (orthonormal when k <= N); 'scaled': the same rows
    times s spanning 1 .. 100 (u = J V is not normalised)."""
    rng = np.random.default_rng(1000 * k + nh + 7 * nx + D + seed)
    us = rows(rng, k, nh)
    ud = np.stack([rows(rng, k, nh) for _ in range(D)])
    vd = np.stack([rows(rng, k, nx) for _ in range(D)])
    if kind == "scaled":
        s = np.logspace(0, 2, k) if k > 1 else np.array([37.0])
        us = us * s[::-1, None]
        ud = ud * s[None, :, None]
        vd = vd * s[None, ::-1, None] * 0.01
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) for a in (us, ud, vd))


def pcs_variants(k):
    """all, the first, the last, and a non-contiguous unsorted subset"""
    out = [None, [0], [k - 1]]
    if k >= 3:
        sub = [k - 1, 0, k // 2] if k < 8 else [k - 2, 3, k // 2, 0, 7]
        out.append(sub)
    return out


def overlap_targets(k, nh, nx, pc, seed=0):
    """A source basis and three targets positioned against its direction a = u_src[pc]: target 0's span contains a (coef_norm = 1), target 1 meets it
    at an overlap of 1e-3 (its first row is 1e-3 a + sqrt(1 - 1e-6) b_1, the others are orthogonal to a), target 2 is generic.  Needs 2 k + 1 <= nh."""
    rng = np.random.default_rng(77 + seed + k)
    us = rows(rng, k, nh)
    a = us[pc]
    q = np.linalg.qr(np.concatenate([a[:, None], rng.standard_normal((nh, 2 * k))], axis=1))[0].T      # q[0] = +-a, the rest orthonormal to it
    b = q[1:]
    t0 = np.concatenate([b[:k - 1], a[None]]) if k > 1 else a[None].copy()
    t1 = b[k:2 * k].copy()
    t1[0] = 1e-3 * a + np.sqrt(1 - 1e-6) * t1[0]
    t2 = rows(rng, k, nh)
    ud = np.stack([t0, t1, t2])
    vd = np.stack([rows(rng, k, nx) for _ in range(3)])
    return tuple(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)) for x in (us, ud, vd))
