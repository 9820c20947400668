"""dpb_geodesic_cotangents and dpb_geodesic_update (csrc/geodesic_chain.hip) against the float64 restatement of tests/_geodesic_ref.py.

Row lengths on both sides of the 4096-element slice and of the group of four (1, 5, 4095, 4096, 4097, 12289 = three slices and one element), m = 1, 2
and 5 interior points, every array once 16-byte aligned and once offset by one float (the 4-byte access path; with an odd row length the rows of one
call alternate between the two).  On small-integer data every operation is exact in either precision and order: cot, P_out and the fp64 sums are
bitwise the restatement's.  On Gaussian data cot and P_out are within one fp32 ulp of it (the same IEEE operations, so in fact equal) and the sums
within D 2^-52 relative, the bound of an fp64 sum of D non-negative terms taken in another order."""
import numpy as np
import pytest
import torch

import _geodesic_ref as R

pytestmark = pytest.mark.gpu

SIZES = [1, 5, 4095, 4096, 4097, 12289]
MS = [1, 2, 5]
ETA, LAM = 0.25, 0.5


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return "cuda:0"


def _place(a, off):
    """the array on the device as a contiguous [rows, D] view that starts `off` floats into a fresh allocation"""
    a = np.ascontiguousarray(a, np.float32)
    buf = torch.zeros(a.size + off + 4, dtype=torch.float32, device=_dev())
    v = buf[off:off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == (4 * off) % 16
    return v


def _empty(rows, D, off):
    return _place(np.full((rows, D), 7.0, np.float32), off)


def _data(kind, m, D, seed):
    rng = np.random.default_rng(seed)
    draw = (lambda *s: rng.integers(-8, 9, s).astype(np.float32)) if kind == "dyadic" else (lambda *s: rng.standard_normal(s).astype(np.float32))
    return draw(m + 2, D), draw(m, D)


def _cot(h, off):
    from diffusion_pullback_amd.engine import geodesic_cotangents
    cot, seg, csq = geodesic_cotangents(_place(h, off), cot=_empty(h.shape[0] - 2, h.shape[1], off))
    return cot.cpu().numpy(), seg.cpu().numpy(), csq.cpu().numpy()


def _upd(P, W, off, eta=ETA, lam=LAM):
    from diffusion_pullback_amd.engine import geodesic_update
    out, stats, xseg = geodesic_update(_place(P, off), _place(W, off), eta, lam, out=_empty(*P.shape, off))
    return out.cpu().numpy(), stats.cpu().numpy(), xseg.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("D", SIZES)
def test_small_integer_data_is_exact(D):
    for m in MS:
        for off in (0, 1):
            h, W = _data("dyadic", m, D, 100 * m + off)
            cot, seg, csq = _cot(h, off)
            rc, rs, rq = R.cotangents_ref(h)
            assert _same_bits(cot, rc) and np.array_equal(seg, rs) and np.array_equal(csq, rq), (m, off)
            out, stats, xseg = _upd(h, W, off)
            ro, rst, rx = R.update_ref(h, W, ETA, LAM)
            assert _same_bits(out, ro) and np.array_equal(stats, rst) and np.array_equal(xseg, rx), (m, off)
            assert (stats[:, 3] == 0).all() and np.array_equal(xseg, seg)          # the curve is its own h here: one segment sum, two kernels


@pytest.mark.parametrize("D", SIZES)
def test_gaussian_data_against_float64(D):
    tol = D * 2.0 ** -52
    close = lambda a, b: (np.abs(a - b) <= tol * np.abs(b)).all()
    ulp = lambda a, b: (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(b))).all()
    for m in MS:
        for off in (0, 1):
            h, W = _data("gauss", m, D, 200 * m + off)
            cot, seg, csq = _cot(h, off)
            rc, rs, rq = R.cotangents_ref(h)
            assert ulp(cot, rc) and close(seg, rs) and close(csq, rq), (m, off)
            for eta, lam in ((0.37, 0.0), (0.011, 1.7)):
                out, stats, xseg = _upd(h, W, off, eta, lam)
                ro, rst, rx = R.update_ref(h, W, eta, lam)
                assert ulp(out, ro) and _same_bits(out[[0, -1]], h[[0, -1]]), (m, off, eta)
                assert close(stats[:, :3], rst[:, :3]) and (stats[:, 3] == 0).all() and close(xseg, rx), (m, off, eta)


@pytest.mark.parametrize("D", [5, 4097, 12289])
def test_a_row_is_a_function_of_its_neighbours_only(D):
    """row i of a 5-point curve is bitwise the middle row of the 3-row call on rows i-1 .. i+1 -- another position, another alignment (D is odd)"""
    m = 3
    h, W = _data("gauss", m, D, 7)
    for off in (0, 1):
        cot, seg, csq = _cot(h, off)
        out, stats, xseg = _upd(h, W, off, 0.3, 0.9)
        for i in range(1, m + 1):
            c1, s1, q1 = _cot(h[i - 1:i + 2], off)
            assert _same_bits(c1[0], cot[i - 1]) and _same_bits(s1, seg[i - 1:i + 1]) and _same_bits(q1, csq[i - 1:i]), (off, i)
            o1, st1, x1 = _upd(h[i - 1:i + 2], W[i - 1:i], off, 0.3, 0.9)
            assert _same_bits(o1[1], out[i]) and _same_bits(st1[0], stats[i - 1]) and _same_bits(x1, xseg[i - 1:i + 1]), (off, i)
    a, b = _cot(h, 0), _cot(h, 1)
    assert all(_same_bits(x, y) for x, y in zip(a, b))                              # and of the alignment not at all
    a, b = _upd(h, W, 0), _upd(h, W, 1)
    assert all(_same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("D", [1, 4097])
def test_eta_zero_returns_the_curve_bitwise(D):
    P, W = _data("gauss", 2, D, 11)
    P[1, 0] = -0.0                                                                  # (p - 0 g would give +0)
    for off in (0, 1):
        out, stats, xseg = _upd(P, W, off, 0.0, 0.8)
        assert _same_bits(out, P) and (stats[:, 2] == 0).all() and (stats[:, 3] == 0).all() and (stats[:, 1] > 0).all()


def test_a_non_finite_row_is_flagged_alone():
    m, D = 5, 4097
    P, W = _data("gauss", m, D, 13)
    clean, cstats, cx = _upd(P, W, 0)
    Wb = W.copy()
    Wb[2, 4096] = np.nan                                                            # interior row 3, in the ragged last group of the second slice
    out, stats, xseg = _upd(P, Wb, 0)
    assert stats[:, 3].tolist() == [0, 0, 1, 0, 0] and np.isnan(out[3]).all()
    keep = [0, 1, 2, 4, 5, 6]
    assert _same_bits(out[keep], clean[keep]) and _same_bits(stats[[0, 1, 3, 4]], cstats[[0, 1, 3, 4]]) and _same_bits(xseg, cx)
    Pb = P.copy()
    Pb[3, 7] = np.inf                                                               # a point of the curve: itself and its two neighbours read it
    out, stats, xseg = _upd(Pb, W, 1)
    assert stats[:, 3].tolist() == [0, 1, 1, 1, 0] and np.isnan(out[2:5]).all()
    assert _same_bits(out[[0, 1, 5, 6]], clean[[0, 1, 5, 6]]) and _same_bits(stats[[0, 4]], cstats[[0, 4]])
    assert np.isfinite(xseg[[0, 1, 4, 5]]).all() and not np.isfinite(xseg[[2, 3]]).any()
    Pe = P.copy()
    Pe[0, 0] = np.nan                                                               # an end point: copied as it is, its neighbour flagged
    out, stats, _ = _upd(Pe, W, 0)
    assert stats[:, 3].tolist() == [1, 0, 0, 0, 0] and np.isnan(out[1]).all() and _same_bits(out[0], Pe[0]) and _same_bits(out[2:], clean[2:])


def test_refused_arguments_leave_the_outputs_untouched():
    from diffusion_pullback_amd import lib as L
    from diffusion_pullback_amd.engine import geodesic_cotangents, geodesic_update
    m, D = 2, 9
    P, W = _data("gauss", m, D, 17)
    Pd, Wd = _place(P, 0), _place(W, 0)
    out = _empty(m + 2, D, 0)
    for kw, word in ((dict(eta=float("nan")), "finite"), (dict(eta=float("inf")), "finite"), (dict(lam=-1.0), "lambda"), (dict(lam=float("nan")), "finite")):
        with pytest.raises(L.DpbError, match=word):
            geodesic_update(Pd, Wd, kw.get("eta", 0.1), kw.get("lam", 0.0), out=out)
    with pytest.raises(L.DpbError, match="overlaps"):
        geodesic_update(Pd, Wd, 0.1, 0.0, out=Pd)
    big = torch.zeros(2 * (m + 2) * D, dtype=torch.float32, device=_dev())
    big[:(m + 2) * D] = Pd.reshape(-1)
    with pytest.raises(L.DpbError, match="overlaps"):                              # P_out starting inside P
        geodesic_update(big[:(m + 2) * D].view(m + 2, D), Wd, 0.1, 0.0, out=big[D:D + (m + 2) * D].view(m + 2, D))
    with pytest.raises(L.DpbError, match="m=0"):
        geodesic_update(Pd[:2], Wd[:1], 0.1, 0.0, out=out[:2])
    with pytest.raises(L.DpbError, match="m=0"):
        geodesic_cotangents(Pd[:2])
    torch.cuda.synchronize()
    assert (out == 7.0).all() and _same_bits(Pd.cpu().numpy(), P) and _same_bits(big[:(m + 2) * D].cpu().numpy(), P.reshape(-1))
    # straight at the C entry points: the scratch
    lib = L.load()
    need = int(lib.dpb_geodesic_update_scratch_bytes(m, D))
    assert need == (m + 1) * 5 * 8 and int(lib.dpb_geodesic_cotangents_scratch_bytes(m, D)) == (m + 1) * 2 * 8
    sc = torch.zeros(64, dtype=torch.float64, device=_dev())
    st, xs = torch.full((m, 4), 7.0, dtype=torch.float64, device=_dev()), torch.full((m + 1,), 7.0, dtype=torch.float64, device=_dev())
    call = lambda scratch, nbytes: lib.dpb_geodesic_update(Pd.data_ptr(), Wd.data_ptr(), out.data_ptr(), 0.1, 0.0, m, D, st.data_ptr(), xs.data_ptr(),
                                                           scratch, nbytes, None)
    assert call(sc.data_ptr(), need - 1) != 0 and b"scratch of" in lib.dpb_last_error()
    assert call(sc.data_ptr() + 4, need) != 0 and b"aligned" in lib.dpb_last_error()
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (st == 7.0).all() and (xs == 7.0).all()
    assert call(sc.data_ptr(), need) == 0                                           # and the call that is in order goes through
    torch.cuda.synchronize()
    ro, rst, rx = R.update_ref(P, W, 0.1, 0.0)
    assert _same_bits(out.cpu().numpy(), ro) and (st[:, 3] == 0).all()
