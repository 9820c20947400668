"""dpb_ddim_step_asym (engine.ddim_step_asym): the asymmetric DDIM step of the h-space guidance edit, on rows of 1 .. 12289 elements.

Yardstick: the float64 evaluation of the same formula on the same fp32 inputs with the fp32 square roots of the fp32 alphas,
    d = e_s - e, eP = e + gP d, eD = e + gD d, P = (x - eP s1a) / sa, out = san P + s1an eD,
elementwise within 8 units of 2^-24 [san / sa (|x| + s1a (|e| + |gP| (|e_s| + |e|))) + s1an (|e| + |gD| (|e_s| + |e|))]: every fp32 operation of the
kernel rounds a quantity bounded by one of these terms, and the numpy fp32 evaluation in the kernel's order stays within 5.0 of that unit over 200
random cases (tests/test_hguide_host.py::test_numpy_fp32_evaluation_within_the_unit, on the CPU); fused multiply-adds only remove roundings."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS, LENS = [1, 3], [1, 5, 4096, 4097, 12289]
GS = [(1.0, 0.0), (1.0, 1.0), (0.0, 0.0), (-2.5, 0.5)]
A_T, A_N = 0.30541, 0.32874          # a step of a 100-step table around t = 696, as fp32 below
U24 = 2.0 ** -24


def _coefs(a_t, a_n):
    a_t, a_n = np.float32(a_t), np.float32(a_n)
    return np.sqrt(a_t), np.sqrt(np.float32(1) - a_t), np.sqrt(a_n), np.sqrt(np.float32(1) - a_n)


def _ref64(x, e, es, a_t, a_n, gP, gD):
    sa, s1a, san, s1an = (np.float64(v) for v in _coefs(a_t, a_n))
    x, e, es = x.astype(np.float64), e.astype(np.float64), es.astype(np.float64)
    gP, gD = np.float64(np.float32(gP)), np.float64(np.float32(gD))
    d = es - e
    eP, eD = e + gP * d, e + gD * d
    P = (x - eP * s1a) / sa
    out = san * P + s1an * eD
    unit = U24 * (san / sa * (np.abs(x) + s1a * (np.abs(e) + abs(gP) * (np.abs(es) + np.abs(e)))) + s1an * (np.abs(e) + abs(gD) * (np.abs(es) + np.abs(e))))
    return out, P, d, unit


def _inputs(n, N, seed, misaligned=False):
    """x, e, e_s [n, N] fp32 on the device; misaligned: views one float into a larger buffer, so that no row is 16-byte aligned when N % 4 == 0"""
    g = torch.Generator().manual_seed(seed)
    mk = lambda s: (s * torch.randn(n * N + 1, generator=g)).to(DEV)
    bufs = [mk(1.0), mk(1.0), mk(1.0)]
    off = 1 if misaligned else 0
    x, e, es = (b[off:off + n * N].view(n, N) for b in bufs)
    es = es.mul_(0.3).add_(e)            # e_s near e, as a shifted net's output is
    return x, e, es


def _call(x, e, es, gP, gD, **kw):
    from diffusion_pullback_amd import engine as E
    return E.ddim_step_asym(x, e, es, A_T, A_N, gP, gD, **kw)


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("N", LENS)
@pytest.mark.parametrize("n", NS)
def test_against_float64(n, N, misaligned):
    x, e, es = _inputs(n, N, 100 + N, misaligned)
    for gP, gD in GS:
        out, x0, stats = _call(x, e, es, gP, gD)
        ref, P, d, unit = _ref64(x.cpu().numpy(), e.cpu().numpy(), es.cpu().numpy(), A_T, A_N, gP, gD)
        r_out = float((np.abs(out.cpu().numpy() - ref) / unit).max())
        r_p = float((np.abs(x0.cpu().numpy() - P) * np.float64(_coefs(A_T, A_N)[2]) / unit).max())       # P carries the first half of the unit
        d32 = (es.cpu().numpy() - e.cpu().numpy()).astype(np.float64)                                      # the fp32 d the kernel forms, summed in fp64
        s2 = (d32 ** 2).sum(axis=1)
        r_s = float((np.abs(stats[:, 0].cpu().numpy() - s2) / s2).max())
        print(f"n={n} N={N} mis={misaligned} g=({gP},{gD}): out {r_out:.2f} units, P {r_p:.2f} units, sum d^2 rel {r_s:.1e}")
        assert r_out <= 8.0 and r_p <= 8.0, (gP, gD, r_out, r_p)
        assert r_s <= 1e-12, r_s
        assert (stats[:, 1] == 0).all()


@pytest.mark.parametrize("N", LENS)
def test_zero_delta_and_zero_g_are_ddim_step_bitwise(N):
    """d == 0 (e_s = e, any g) and g = (0, 0) (any e_s): dpb_ddim_step on (x, e), out and x0, bit for bit"""
    import ctypes as C
    from diffusion_pullback_amd import lib as L
    n = 3
    x, e, es = _inputs(n, N, 7 + N)
    x, e, es = x.contiguous(), e.contiguous(), es.contiguous()
    lib = L.load()
    want, want0 = torch.empty_like(x), torch.empty_like(x)
    L.check(lib.dpb_ddim_step(x.data_ptr(), e.data_ptr(), want.data_ptr(), want0.data_ptr(), x.numel(), A_T, A_N,
                              C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    for gP, gD, s in [(1.0, 0.0, e), (-2.5, 0.5, e), (0.0, 0.0, es)]:
        out, x0, stats = _call(x, e, s, gP, gD)
        assert torch.equal(out, want) and torch.equal(x0, want0), (N, gP, gD)
        if s is e:
            assert (stats[:, 0] == 0).all()
    # in place: out aliasing x
    xc = x.clone()
    out, _, _ = _call(xc, e, es, 1.0, 0.0, out=xc, return_x0=False)
    assert out.data_ptr() == xc.data_ptr() and torch.equal(xc, _call(x, e, es, 1.0, 0.0)[0])


@pytest.mark.parametrize("N", LENS)
def test_row_is_the_same_alone_and_in_a_stack_and_nan_rows_are_flagged(N):
    x, e, es = _inputs(3, N, 31 + N)
    out, x0, stats = _call(x, e, es, -2.5, 0.5)
    for b in range(3):
        o1, p1, s1 = _call(x[b:b + 1].clone(), e[b:b + 1].clone(), es[b:b + 1].clone(), -2.5, 0.5)
        assert torch.equal(o1[0], out[b]) and torch.equal(p1[0], x0[b]) and torch.equal(s1[0], stats[b]), (N, b)
    for which in range(3):
        bad = [t.clone() for t in (x, e, es)]
        bad[which][1, N // 2] = float("nan") if which != 1 else float("inf")
        o2, p2, s2 = _call(*bad, -2.5, 0.5)
        assert s2[:, 1].tolist() == [0.0, 1.0, 0.0]
        assert torch.isnan(o2[1]).all() and torch.isnan(p2[1]).all()
        for b in (0, 2):
            assert torch.equal(o2[b], out[b]) and torch.equal(p2[b], x0[b]) and torch.equal(s2[b], stats[b]), (N, which, b)


def test_refusals():
    import ctypes as C
    from diffusion_pullback_amd import DpbError, lib as L
    x, e, es = _inputs(2, 5, 3)
    from diffusion_pullback_amd import engine as E
    for a_t, a_n, gP, gD in [(0.0, 0.5, 1, 0), (0.5, 1.5, 1, 0), (float("nan"), 0.5, 1, 0), (0.5, 0.5, float("inf"), 0), (0.5, 0.5, 1, float("nan"))]:
        with pytest.raises(DpbError):
            E.ddim_step_asym(x, e, es, a_t, a_n, gP, gD)
    lib = L.load()
    stats = torch.empty(2, 2, dtype=torch.float64, device=DEV)
    scratch = torch.empty(64, dtype=torch.float64, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = lambda **k: [k.get("x", x.data_ptr()), e.data_ptr(), es.data_ptr(), k.get("out", x.data_ptr()), None, k.get("n", 2), k.get("N", 5), 0.5, 0.6, 1.0, 0.0,
                        stats.data_ptr(), k.get("scratch", scratch.data_ptr()), k.get("bytes", 512), st]
    for kw in (dict(x=None), dict(out=None), dict(n=0), dict(N=0), dict(bytes=8), dict(scratch=scratch.data_ptr() + 4)):
        assert lib.dpb_ddim_step_asym(*args(**kw)) != 0, kw
    out, _, _ = E.ddim_step_asym(x, e, es, 0.5, 0.6)                   # the next call is unaffected
    assert torch.isfinite(out).all()
