"""Replay of the draw sequence the reference's local_pca_zt / local_pca_xt make on the global CPU generator after torch.manual_seed(rng_seed):
one torch.randn_like of [memory_bound, C, H, W] per chunk of memory_bound samples (src/utils/utils.py:917-925, src/models/ddpm/diffusion.py:397-400),
then torch.pca_lowrank's R = torch.randn(min(N, D), q).  One draw of [N, C, H, W] need not be the same stream (the CPU generator fills
normals in vectors of 16, so a chunk whose element count is no multiple of 16 ends differently), hence the chunked replay.  The fixtures store the noise and R when small, and always their sums;
the replay is checked against both.  Also the integer restatement of the device noise kernel's generator (Philox4x32-10 and the Box-Muller
mapping include/dpb.h writes down), used by the host and GPU tests."""
import math

import torch

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: 4 words, key: 2 words -> 4 words"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def unit_open(w):
    """include/dpb.h: u(w) = ((w >> 9) + 0.5) * 2^-23"""
    return ((w >> 9) + 0.5) * 2.0 ** -23


def philox_normals(seed, index, n):
    """the n unnormalised normals of sample `index` under `seed`, in fp64 (include/dpb.h, dpb_perturb_unit)"""
    out = []
    key = (seed & MASK, (seed >> 32) & MASK)
    for c in range((n + 3) // 4):
        w = philox4x32_10((index & MASK, (index >> 32) & MASK, c & MASK, (c >> 32) & MASK), key)
        for p in (0, 1):
            r = math.sqrt(-2.0 * math.log(unit_open(w[2 * p])))
            a = 2.0 * math.pi * unit_open(w[2 * p + 1])
            out += [r * math.cos(a), r * math.sin(a)]
    return torch.tensor(out[:n], dtype=torch.float64)


def _sums(t):
    return t.double().sum().item(), t.double().abs().sum().item()


def _close(got, want):
    return math.isclose(got[0], want[0], rel_tol=1e-12, abs_tol=1e-9) and math.isclose(got[1], want[1], rel_tol=1e-12)


def replay(case, shape, generator=None):
    """(noise [N, *shape], R [min(N, D), q]) of a local-PCA fixture case as the reference drew them.  generator=None replays on the GLOBAL CPU
    generator after torch.manual_seed(rng_seed), leaving it where the reference's next draw would come from."""
    n, mb = case["n"], case["memory_bound"]
    if generator is None:
        torch.manual_seed(case["rng_seed"])
    else:
        generator.manual_seed(case["rng_seed"])
    noise = torch.cat([torch.randn(mb, *shape, generator=generator) for _ in range(n // mb)], dim=0)
    R = torch.randn(min(n, case["d"]), case["q"], generator=generator)
    assert _close(_sums(noise), (case["noise_sum"], case["noise_abs_sum"])), "the noise does not replay"
    assert _close(_sums(R), (case["R_sum"], case["R_abs_sum"])), "R does not replay"
    if "noise" in case:
        assert torch.equal(noise, case["noise"]) and torch.equal(R, case["R"]), "the stored noise / R differ from the replay"
    return noise, R


def position_at_R(case, shape):
    """the test's set-up of a golden call with injected noise: seed the global CPU generator and consume the reference's noise draws, so that the
    next draw (the method's torch.randn for R) is the reference's R.  Returns the noise."""
    n, mb = case["n"], case["memory_bound"]
    torch.manual_seed(case["rng_seed"])
    noise = torch.cat([torch.randn(mb, *shape) for _ in range(n // mb)], dim=0)
    assert _close(_sums(noise), (case["noise_sum"], case["noise_abs_sum"])), "the noise does not replay"
    return noise


def reference_pairing(u):
    """the h-space direction utils.local_pca_zt differentiates for row i of its vT: row i of `u.view(q, C, H, W)` (utils.py:960), the row-major
    view of u [D, q] as [q, D] -- NOT column i of u unless q = 1.  Returns W [q, D]."""
    d, q = u.shape
    return u.contiguous().view(q, d)
