"""GPU tests of the global h-space PCA (dpb_pca_lowrank; bind()-attached global_pca_zt / inv_jac_zt): the reference's goldens, the raw
entry point against the fp64 Gram restatement (tests/_pca_ref.py) in both orientations, past 4 GiB of H, reproducibility, the 2-D u
extension of inv_jac_zt, error paths and isolation from the pullback."""
import os

import pytest
import torch

from _pca_ref import golden_zt, pca_lowrank_gram
from _util import abs_cos, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class _Unet:
    """stands in for the diffusers module bind() patches: only state_dict() is read"""

    def __init__(self, p):
        self._p = p

    def state_dict(self):
        return self._p


def _bound(g, dtype=torch.float32, max_batch=5, max_rank=4):
    from diffusion_pullback_amd import bind
    from oracle import unet_sd
    cfg = unet_sd.SDConfig(**g["cfg"])
    p = unet_sd.init_params(cfg, seed=g["seed"], gain=g["gain"])
    unet = _Unet(p)
    impl = bind(unet, "sd", cfg, dtype=dtype, device=DEV, max_batch=max_batch, max_rank=max_rank, verbose=False)
    return unet, impl


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_global_pca_zt_golden(dtype):
    g = load_golden("pca_zt_tiny.pt")
    unet, _ = _bound(g, dtype)
    for c in g["pca"]:
        torch.manual_seed(c["rng_seed"])                   # the reference's R comes from the global CPU generator (pca_device='cpu')
        u, s = unet.global_pca_zt(golden_zt(c), g["t"], g["ctx"], op=c["op"], block_idx=c["idx"], memory_bound=c["memory_bound"], pca_rank=c["q"])
        assert u.device.type == "cpu" and s.device.type == "cpu" and u.dtype == torch.float32
        assert tuple(u.shape) == tuple(c["u"].shape) and tuple(s.shape) == (c["q"],)
        cos = abs_cos(u.T, c["u"].T)
        srel = ((s.double() - c["s"].double()).abs() / c["s"].double()).max().item()
        if dtype == torch.float32:
            assert srel <= 1e-4, (c["n"], c["q"], srel)
            assert cos.min() >= 0.9999, (c["n"], c["q"], cos)
        else:
            assert srel <= 2e-2, (c["n"], c["q"], srel)
            assert cos[0] >= 0.99, (c["n"], c["q"], cos)


def test_inv_jac_zt_golden():
    g = load_golden("pca_zt_tiny.pt")
    unet, _ = _bound(g)
    for c in g["inv"]:
        vT = unet.inv_jac_zt(g["z"], g["t"], g["ctx"], op=c["op"], block_idx=c["idx"], u=c["u"], perturb_h=c["perturb_h"])
        assert tuple(vT.shape) == tuple(c["vT"].shape)
        assert abs_cos(vT, c["vT"]).min() >= 0.9999 and (vT.cpu() * c["vT"]).sum() > 0, c["name"]


def _synthetic(n, d, rank, seed, decades=2.0, mean=3.0, device=DEV):
    """H [n, d] fp32 on the device: a decaying spectrum (s_i = 10^(-decades i / rank)) on top of a large column mean, plus small noise"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    L = torch.randn(n, rank, generator=g) * torch.logspace(0, -decades, rank)
    Rm = torch.randn(rank, d, generator=g) / d ** 0.5
    mu = mean + torch.rand(d, generator=g)
    H = (L.to(device) @ Rm.to(device)) * 10.0 + mu.to(device)
    H += 1e-4 * torch.randn(n, d, generator=g).to(device)
    return H.contiguous()


def _check_raw(H, q, niter, seed, s_tol=1e-4, cos_tol=0.999):
    from diffusion_pullback_amd.engine import pca_lowrank
    n, d = H.shape
    R = torch.randn(min(n, d), q, generator=torch.Generator().manual_seed(seed))
    u, s = pca_lowrank(H, R, q, niter)
    torch.cuda.synchronize()
    ur, sr = pca_lowrank_gram(H.cpu(), R, q, niter)
    assert torch.isfinite(u).all() and torch.isfinite(s).all()
    srel = ((s.cpu().double() - sr.double()).abs() / sr.double()).max().item()
    cos = abs_cos(u, ur)
    assert srel <= s_tol, (n, d, q, niter, srel)
    # a singular vector is defined (to rounding) where its singular value stands apart from its neighbours' by >= 1 %
    sd = sr.double()
    gap = torch.full_like(sd, float("inf"))
    gap[1:] = torch.minimum(gap[1:], (sd[:-1] - sd[1:]) / sd[1:])
    gap[:-1] = torch.minimum(gap[:-1], (sd[:-1] - sd[1:]) / sd[:-1])
    sep = gap >= 1e-2
    assert cos[sep].min() >= cos_tol if sep.any() else True, (n, d, q, niter, cos[sep].min().item())
    nrm = u.double().norm(dim=1).cpu()
    assert (nrm - 1).abs().max() <= 1e-4
    return u, s


@pytest.mark.parametrize("n,d", [(300, 4100), (3000, 400)])            # N < D and N >= D; 4100 and 400: ragged against every tile
@pytest.mark.parametrize("q", [1, 5, 50, 100, 128])
@pytest.mark.parametrize("niter", [0, 2, 5])
def test_pca_lowrank_raw_against_fp64(n, d, q, niter):
    H = _synthetic(n, d, rank=min(n, d, 160), seed=q * 10 + niter)
    _check_raw(H, q, niter, seed=1000 + q)


def test_pca_lowrank_raw_ragged_d():
    H = _synthetic(77, 1237, rank=60, seed=5)                                 # 1237: not a multiple of 16, 32 or 128
    _check_raw(H, 20, 3, seed=6)


def test_pca_lowrank_full_size_sd15_mid():
    """D = 1280 * 8 * 8 = 81 920 features of the SD-1.5 mid tap, N = 600 samples, q = 100, niter = 5"""
    H = _synthetic(600, 81920, rank=200, seed=7)
    _check_raw(H, 100, 5, seed=8)


def test_pca_lowrank_beyond_4gib():
    """H fp32 at the up3 tap (D = 320 * 64 * 64 = 1 310 720) with N = 900: 4.7 GB, past every 32-bit element offset"""
    from diffusion_pullback_amd.engine import pca_lowrank
    n, d, r, q = 900, 1310720, 6, 4
    g = torch.Generator().manual_seed(11)
    L = torch.randn(n, r, generator=g) * torch.tensor([8.0, 4.0, 2.0, 1.0, 0.5, 0.25])
    Rm = torch.randn(r, d, generator=g) / d ** 0.5
    H = L.to(DEV) @ Rm.to(DEV)
    H += 1.0
    assert H.numel() * 4 > 4 * 2 ** 30
    R = torch.randn(n, q, generator=torch.Generator().manual_seed(12))
    u, s = pca_lowrank(H, R, q, 1)
    # fp64 restatement through the factors: Hc = (L - mean L) Rm
    Lc = (L.double() - L.double().mean(0, keepdim=True))
    Rd = Rm.double()

    def orth(W):
        lam, E = torch.linalg.eigh(W @ W.T)
        lam, E = lam.flip(0), E.flip(1)
        return (E.T @ W) / lam.sqrt()[:, None], lam.sqrt(), E
    # N < D: A = Hc^T; rows of Q live in D-space
    Q, _, _ = orth(((Lc.T @ R.double()).T @ Rd))              # (A R)^T = R^T Hc = (R^T Lc) Rm
    Q, _, _ = orth((Q @ Rd.T) @ Lc.T)                         # (A^H Q)^T = Q Hc^T
    Q, _, _ = orth((Q @ Lc) @ Rd)                             # (A Q)^T = Q Hc
    B = (Q @ Rd.T) @ Lc.T
    _, S, E = orth(B)
    ur = E.T @ Q
    assert ((s.cpu().double() - S).abs() / S).max() <= 1e-4
    cos = abs_cos(u, ur.float())
    assert cos.min() >= 0.999, cos
    # the last rows of H (beyond 4 GiB) enter the result: the tail of u matches too
    tail = slice(d - 4096, d)
    assert abs_cos(u[:, tail], ur[:, tail].float()).min() >= 0.99


def test_pca_lowrank_bitwise_reproducible():
    from diffusion_pullback_amd.engine import pca_lowrank
    for n, d in [(600, 81920), (3000, 400)]:
        H = _synthetic(n, d, rank=150, seed=21)
        R = torch.randn(min(n, d), 64, generator=torch.Generator().manual_seed(22))
        u1, s1 = pca_lowrank(H, R, 64, 5)
        u2, s2 = pca_lowrank(H, R, 64, 5)
        assert torch.equal(u1, u2) and torch.equal(s1, s2)


def _raw(H, R, q, niter, scratch):
    """dpb_pca_lowrank itself with the caller's scratch -> (return value, u, s)"""
    import ctypes as C

    from diffusion_pullback_amd import lib as L
    lib = L.load()
    n, d = H.shape
    u = torch.empty(q, d, dtype=torch.float32, device=DEV)
    s = torch.empty(q, dtype=torch.float32, device=DEV)
    r = lib.dpb_pca_lowrank(H.data_ptr(), n, d, R.data_ptr(), q, niter, u.data_ptr(), s.data_ptr(), scratch.data_ptr(), scratch.numel(),
                            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return r, u, s


@pytest.mark.parametrize("q", [5, 50, 128])
def test_pca_lowrank_non_finite_input_is_all_nan_and_leaves_no_state(q):
    """include/dpb.h: one NaN or inf anywhere in H or R -> u and s all NaN, return 0 (every factorisation is dpb_orth, whose rule this is); the next
    clean call on the same scratch returns the bits of a clean call on a fresh scratch.  Exact: NaN masks and bit equality."""
    from diffusion_pullback_amd import lib as L
    n, d, niter = 300, 4100, 2
    H = _synthetic(n, d, rank=160, seed=q)
    R = torch.randn(n, q, generator=torch.Generator().manual_seed(2000 + q)).to(DEV)
    need = int(L.load().dpb_pca_scratch_bytes(q, n, d))
    fresh = lambda: torch.empty(need, dtype=torch.uint8, device=DEV)
    r0, u0, s0 = _raw(H, R, q, niter, fresh())
    assert r0 == 0 and torch.isfinite(u0).all() and torch.isfinite(s0).all()
    scratch = fresh()
    for what, where, val in [("H", (n - 1, d - 1), float("nan")), ("H", (7, 1234), float("inf")), ("R", (n // 2, q - 1), float("nan"))]:
        Hb, Rb = H.clone(), R.clone()
        (Hb if what == "H" else Rb)[where] = val
        r, u, s = _raw(Hb, Rb, q, niter, scratch)
        assert r == 0, (what, val, L.load().dpb_last_error())
        assert torch.isnan(s).all(), (what, val, "s", s[:4].tolist())
        assert torch.isnan(u).all(), (what, val, "u", int(torch.isnan(u).sum()), u.numel())
        r, u, s = _raw(H, R, q, niter, scratch)
        assert r == 0 and torch.equal(u.view(torch.int32), u0.view(torch.int32)) and torch.equal(s.view(torch.int32), s0.view(torch.int32)), \
            (what, val, "the clean call on the same scratch differs")


def test_inv_jac_zt_2d_u_equals_per_column_calls():
    g = load_golden("pca_zt_tiny.pt")
    unet, _ = _bound(g, max_rank=3)
    U = torch.randn(1024, 7, generator=torch.Generator().manual_seed(31))   # 7 columns: three adjoint chunks at max_rank = 3
    V = unet.inv_jac_zt(g["z"], g["t"], g["ctx"], op="mid", block_idx=0, u=U)
    assert tuple(V.shape) == (7, 256)
    for i in range(7):
        vi = unet.inv_jac_zt(g["z"], g["t"], g["ctx"], op="mid", block_idx=0, u=U[:, i])
        assert torch.allclose(V[i], vi[0], atol=1e-6, rtol=1e-5), i
    assert torch.allclose(V.norm(dim=1).cpu(), torch.ones(7), atol=1e-5)


def test_pca_error_paths_leave_the_engine_usable():
    from diffusion_pullback_amd import DpbError
    g = load_golden("pca_zt_tiny.pt")
    unet, impl = _bound(g)
    c = g["pca"][1]
    zt = golden_zt(c)
    for q in (129, zt.shape[0], zt.shape[0] + 3):
        with pytest.raises(ValueError, match="pca_rank"):
            unet.global_pca_zt(zt, g["t"], g["ctx"], op="mid", block_idx=0, pca_rank=q)
    with pytest.raises(ValueError, match="sample size should be 1"):
        unet.inv_jac_zt(zt[:2], g["t"], g["ctx"], op="mid", block_idx=0, u=c["u"][:, 0])
    from diffusion_pullback_amd.engine import pca_lowrank
    H = torch.randn(10, 50, device=DEV)
    with pytest.raises(DpbError, match="q outside"):
        pca_lowrank(H, torch.randn(10, 129), 129, 1)
    with pytest.raises(DpbError, match="N - 1"):
        pca_lowrank(H, torch.randn(10, 10), 10, 1)
    torch.manual_seed(c["rng_seed"])
    u, s = unet.global_pca_zt(zt, g["t"], g["ctx"], op="mid", block_idx=0, memory_bound=c["memory_bound"], pca_rank=c["q"])
    assert abs_cos(u.T, c["u"].T).min() >= 0.9999


def test_pullback_bits_unchanged_by_a_pca_call():
    g = load_golden("pca_zt_tiny.pt")
    unet, impl = _bound(g)
    V0 = torch.linalg.qr(torch.randn(256, 3, generator=torch.Generator().manual_seed(41)))[0].T.contiguous()
    r1 = [t.clone() for t in impl.pullback_fixed(g["z"], g["t"], g["ctx"], "mid", 0, 3, 4, V0)]
    c = g["pca"][2]
    torch.manual_seed(c["rng_seed"])
    unet.global_pca_zt(golden_zt(c), g["t"], g["ctx"], op="mid", block_idx=0, memory_bound=c["memory_bound"], pca_rank=c["q"])
    unet.inv_jac_zt(g["z"], g["t"], g["ctx"], op="mid", block_idx=0, u=c["u"][:, 0])
    r2 = impl.pullback_fixed(g["z"], g["t"], g["ctx"], "mid", 0, 3, 4, V0)
    for a, b in zip(r1, r2):
        assert torch.equal(a, b)
