"""fp64 CPU restatement of what dpb_pca_lowrank computes: torch.pca_lowrank(H, q, center=True, niter) (torch._lowrank._svd_lowrank +
get_approximate_basis) with every QR replaced by the Gram orthonormalisation of dpb_orth -- G = W W^T, G = E diag(lam) E^T, rows
diag(lam)^-1/2 E^T W -- which spans the same space, and svd(B) by the same Gram eigen-decomposition.  Returns u [q, D] (rows; sign
arbitrary) and s [q] (descending)."""
import math

import torch


def golden_zt(case):
    """the samples zt of a pca_zt_tiny.pt case, redrawn from their seed on the CPU generator (the fixture stores the seed and two sums,
    not the [N, 4, 8, 8] tensor)"""
    zt = torch.randn(case["n"], 4, 8, 8, generator=torch.Generator().manual_seed(case["zt_seed"]))
    if "zt_sum" in case:
        s, a = zt.double().sum().item(), zt.double().abs().sum().item()
        assert math.isclose(s, case["zt_sum"], rel_tol=1e-12, abs_tol=1e-9) and math.isclose(a, case["zt_abs_sum"], rel_tol=1e-12), "zt does not redraw"
    return zt


def golden_R(case):
    """the Gaussian matrix R of a pca_zt_tiny.pt case: stored, or redrawn as torch.pca_lowrank drew it after torch.manual_seed(rng_seed)"""
    if "R" in case:
        return case["R"]
    g = torch.Generator().manual_seed(case["rng_seed"])
    R = torch.randn(min(case["n"], case["d"]), case["q"], generator=g)
    s, a = R.double().sum().item(), R.double().abs().sum().item()
    assert math.isclose(s, case["R_sum"], rel_tol=1e-12, abs_tol=1e-9) and math.isclose(a, case["R_abs_sum"], rel_tol=1e-12), "R does not redraw"
    return R


def gram_orth(W):
    """W [k, n] -> (V [k, n] orthonormal rows spanning W's rows, sigma [k] singular values of W, E [k, k] Gram eigenvectors), descending"""
    lam, E = torch.linalg.eigh(W @ W.T)
    lam, E = lam.flip(0), E.flip(1)
    sig = lam.clamp_min(0).sqrt()
    return (E.T @ W) / sig[:, None], sig, E


def pca_lowrank_gram(H, R, q, niter):
    H = H.double()
    R = R.double()
    Hc = H - H.mean(0, keepdim=True)
    n, d = Hc.shape
    A = Hc.T if n < d else Hc                    # _svd_lowrank: transpose when m < n
    Q, _, _ = gram_orth((A @ R).T)               # rows = Q^T
    for _ in range(niter):
        Q, _, _ = gram_orth(Q @ A)               # (A^H Q)^T
        Q, _, _ = gram_orth(Q @ A.T)             # (A Q)^T
    B = Q @ A                                    # Q^H A [q, cols of A]
    Vb, S, Ub = gram_orth(B)                     # B = Ub diag(S) Vb
    if n < d:                                    # swapped back: the reference's u is Q Ub
        return (Ub.T @ Q).float(), S.float()
    return Vb.float(), S.float()
