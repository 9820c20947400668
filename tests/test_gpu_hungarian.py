"""geometry.hungarian_mean (dpb_matched_mean, csrc/hungarian.hip) on the GPU against tests/_hungarian_ref.py, the numpy float64 restatement with scipy's
solver, on the same fp32 inputs.

Bars.  Planted sets (the optimum's gap is wide): perm and sign EXACTLY the restatement's, every element of Y within 2^-23 |Y_ref| + 1e-12 of the
restatement's (Y is one fp32 rounding of an fp64 sum).  Gaussian sets (the optimum is unique but its gap is not controlled): each basis's device
assignment, costed on the RESTATEMENT's matrix, within 1e-9 relative of scipy's optimum, and Y within the bar above of the restatement evaluated with
the device's perm / sign."""
import functools

import numpy as np
import pytest
import torch

import _hungarian_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLANTED = [(7, 17, 257, 0.5), (33, 50, 4099, 1.0), (5, 128, 513, 1.0)]
GAUSSIAN = [(7, 17, 257), (33, 50, 4099)]


def _geo():
    from diffusion_pullback_amd import geometry
    return geometry


def _dev(a):
    return torch.tensor(np.asarray(a), device=DEV)          # (a copy: the cached sets are read-only)


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _planted(b, k, n, sigma):
    a, y, perm, sign = R.planted_set(np.random.default_rng(100 * k + b), b, k, n, sigma)
    a.setflags(write=False)
    return a, perm, sign


@functools.lru_cache(maxsize=None)
def _planted_ref(b, k, n, sigma, distance):
    return R.hungarian_mean_ref(_planted(b, k, n, sigma)[0], distance=distance)


@functools.lru_cache(maxsize=None)
def _gaussian(b, k, n):
    a = R.gaussian_set(np.random.default_rng(10 * k + b), b, k, n)
    a.setflags(write=False)
    return a


def _y_err(Y, Yr):
    """the largest excess of |Y - Y_ref| over the bar 2^-23 |Y_ref| + 1e-12 (<= 0 passes), and the largest error in units of 2^-23 |Y_ref|"""
    Y, Yr = _np(Y).astype(np.float64), np.asarray(Yr, dtype=np.float64)
    err = np.abs(Y - Yr)
    return float((err - (2.0 ** -23 * np.abs(Yr) + 1e-12)).max()), float((err / (2.0 ** -23 * np.abs(Yr) + 1e-12)).max())


@pytest.mark.parametrize("distance", R.DISTANCES)
@pytest.mark.parametrize("b,k,n,sigma", PLANTED)
def test_planted_sets_match_the_restatement_exactly(b, k, n, sigma, distance):
    a, perm, sign = _planted(b, k, n, sigma)
    Yr, ir = _planted_ref(b, k, n, sigma, distance)
    Y, info = _geo().hungarian_mean(_dev(a), distance=distance)
    excess, units = _y_err(Y, Yr)
    cost_err = np.abs(info["cost"] - ir["cost"]).max() / np.abs(ir["cost"]).max()
    w_err = np.abs(_np(info["weight"]) - ir["weight"]).max()
    print(f"planted B = {b}, k = {k}, N = {n}, {distance}: {info['sweeps']} sweeps, changed {info['changed']}; Y error {units:.3f} of the bar, "
          f"cost relative error {cost_err:.2e}, weight error {w_err:.2e}")
    assert (_np(info["perm"]) == ir["perm"]).all() and (_np(info["sign"]) == ir["sign"]).all()
    assert (ir["perm"] == perm).all() and (ir["sign"] == sign).all()
    assert excess <= 0
    assert info["converged"] and info["sweeps"] == ir["sweeps"] == 2 and info["changed"] == ir["changed"]
    assert info["cost"].shape == (2, b) and cost_err <= 1e-9               # (the Gaussian sets' bar: an fp32 ulp of one anchor element moves an overlap by 2^-24 / N)
    assert w_err <= 2.0 ** -23                                             # (fp32 output of an fp64 mean of overlaps)


@pytest.mark.parametrize("distance", R.DISTANCES)
@pytest.mark.parametrize("b,k,n", GAUSSIAN)
def test_gaussian_sets_reach_the_optimum(b, k, n, distance):
    a = _gaussian(b, k, n)
    xh = R.unit_rows(a)
    Y1, i1 = _geo().hungarian_mean(_dev(a), distance=distance, max_sweeps=1)
    # sweep 1 on the restatement's matrix: the device's assignment costs what scipy's optimum costs
    pr, sr, total, d = R.sweep(xh, xh[0], distance)
    perm, sign = _np(i1["perm"]), _np(i1["sign"])
    assert (np.sort(perm, axis=1) == np.arange(k)).all()
    own = np.array([d[m][np.arange(k), perm[m]].sum() for m in range(b)])
    gap = np.abs(own - total) / np.abs(total)
    print(f"gaussian B = {b}, k = {k}, N = {n}, {distance}: sweep 1 cost against scipy's optimum {gap.max():.2e} relative; "
          f"{int((perm != pr).sum())} entries differ from scipy's permutation")
    assert gap.max() <= 1e-9
    c = R.overlaps(xh, xh[0])
    assert (sign == np.where(np.take_along_axis(c, perm[:, :, None].astype(np.int64), axis=2)[:, :, 0] < 0, -1, 1)).all()
    assert _y_err(Y1, R.mean_with_f64(xh, perm, sign))[0] <= 0
    assert not i1["converged"] and i1["sweeps"] == 1 and i1["changed"] == [b * k]
    # to convergence: the last sweep's assignment is optimal against the anchor it was computed from, and Y is the mean of that assignment
    Y, info = _geo().hungarian_mean(_dev(a), distance=distance)
    perm, sign = _np(info["perm"]), _np(info["sign"])
    print(f"    converged {info['converged']} after {info['sweeps']} sweeps, changed {info['changed']}")
    assert info["converged"] and info["changed"][-1] == 0 and 2 <= info["sweeps"] <= 20
    assert _y_err(Y, R.mean_with_f64(xh, perm, sign))[0] <= 0
    _, _, total, d = R.sweep(xh, _np(Y).astype(np.float64), distance)       # (converged: Y is also the last sweep's anchor, bitwise)
    own = np.array([d[m][np.arange(k), perm[m]].sum() for m in range(b)])
    assert (np.abs(own - total) / np.abs(total)).max() <= 1e-9
    assert np.abs(info["cost"][-1] - own).max() / np.abs(own).max() <= 1e-9
    assert info["cost"].shape == (info["sweeps"], b)


@pytest.mark.parametrize("distance", R.DISTANCES)
def test_one_basis_is_its_own_mean(distance):
    a = _gaussian(7, 17, 257)[:1]
    Y, info = _geo().hungarian_mean(_dev(a), distance=distance)
    assert (_np(info["perm"])[0] == np.arange(17)).all() and (_np(info["sign"]) == 1).all()
    assert _y_err(Y, R.unit_rows(a[0]))[0] <= 0
    assert info["converged"] and info["sweeps"] == 2


def test_row_scaling_changes_nothing_but_rounding():
    a = _gaussian(7, 17, 257)
    scale = np.random.default_rng(5).uniform(0.5, 2.0, size=(7, 17, 1)).astype(np.float32)
    scale = 2.0 ** np.round(np.log2(scale))                                 # powers of two: xhat is then the same fp64 number
    _, i0 = _geo().hungarian_mean(_dev(a))
    _, i1 = _geo().hungarian_mean(_dev(a * scale.astype(np.float32)))
    assert (_np(i0["perm"]) == _np(i1["perm"])).all() and (_np(i0["sign"]) == _np(i1["sign"])).all()
    b, k, n, sigma = PLANTED[0]
    p = _planted(b, k, n, sigma)[0]
    _, i2 = _geo().hungarian_mean(_dev(p * np.random.default_rng(6).uniform(0.5, 2.0, size=(b, k, 1)).astype(np.float32)))
    assert (_np(i2["perm"]) == _planted(b, k, n, sigma)[1]).all() and (_np(i2["sign"]) == _planted(b, k, n, sigma)[2]).all()


def test_explicit_anchor_and_init():
    a = _gaussian(7, 17, 257)
    xh = R.unit_rows(a)
    Y0, i0 = _geo().hungarian_mean(_dev(a), init=3, max_sweeps=1)
    Y1, i1 = _geo().hungarian_mean(_dev(a), anchor=_dev(a[3]), max_sweeps=1)
    assert torch.equal(Y0, Y1) and torch.equal(i0["perm"], i1["perm"]) and torch.equal(i0["sign"], i1["sign"])
    assert (_np(i0["perm"])[3] == np.arange(17)).all()
    anchor = np.linalg.qr(np.random.default_rng(8).standard_normal((257, 17)))[0].T.astype(np.float32)
    Y2, i2 = _geo().hungarian_mean(_dev(a), anchor=_dev(anchor), max_sweeps=1)
    _, _, total, d = R.sweep(xh, anchor.astype(np.float64), "1/cosine")
    perm = _np(i2["perm"])
    own = np.array([d[m][np.arange(17), perm[m]].sum() for m in range(7)])
    assert (np.abs(own - total) / total).max() <= 1e-9
    assert _y_err(Y2, R.mean_with_f64(xh, perm, _np(i2["sign"])))[0] <= 0


@pytest.mark.parametrize("n", [257, 260])
def test_unaligned_view(n):
    """rows that start 4 bytes past a 16-byte boundary (and, for N = 257, rows of odd length): the same numbers as the aligned copy, bitwise"""
    a = _gaussian(7, 17, 257) if n == 257 else R.gaussian_set(np.random.default_rng(9), 5, 6, 260)
    flat = torch.zeros(a.size + 1, dtype=torch.float32, device=DEV)
    flat[1:] = _dev(a).flatten()
    view = flat[1:].view(*a.shape)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    Y0, i0 = _geo().hungarian_mean(_dev(a))
    Y1, i1 = _geo().hungarian_mean(view)
    assert torch.equal(Y0, Y1) and torch.equal(i0["perm"], i1["perm"]) and torch.equal(i0["sign"], i1["sign"])
    assert (i0["cost"] == i1["cost"]).all()


def test_a_zero_row_raises_naming_the_basis():
    a = np.array(_gaussian(7, 17, 257))
    a[4, 2] = 0.0
    with pytest.raises(ValueError, match=r"indices \[4\]"):
        _geo().hungarian_mean(_dev(a))
    Y, info = _geo().hungarian_mean(_dev(a), check=False)
    assert info["degenerate"] == [4] and (_np(info["perm"])[4] == -1).all() and torch.isnan(Y).all()
    assert (np.sort(_np(info["perm"])[[0, 1, 2, 3, 5, 6]], axis=1) == np.arange(17)).all()
    a[4, 2] = np.inf
    with pytest.raises(ValueError, match=r"indices \[4\]"):
        _geo().hungarian_mean(_dev(a))


def test_bad_arguments():
    a = _dev(_gaussian(7, 17, 257))
    with pytest.raises(ValueError, match="distance"):
        _geo().hungarian_mean(a, distance="euclid")
    with pytest.raises(ValueError, match="init"):
        _geo().hungarian_mean(a, init=7)
    with pytest.raises(ValueError, match="128"):
        _geo().hungarian_mean(torch.zeros(2, 129, 200, device=DEV))


@pytest.mark.parametrize("b,k,n", [(7, 17, 257), (5, 128, 513)])
def test_batch_invariant_and_reproducible(b, k, n):
    a = _gaussian(b, k, n) if k == 17 else _planted(b, k, n, 1.0)[0]
    anchor = _dev(a[0])
    Y, info = _geo().hungarian_mean(_dev(a), anchor=anchor, max_sweeps=1)
    Y2, info2 = _geo().hungarian_mean(_dev(a), anchor=anchor, max_sweeps=1)
    assert torch.equal(Y, Y2) and torch.equal(info["perm"], info2["perm"]) and torch.equal(info["sign"], info2["sign"])
    assert (info["cost"] == info2["cost"]).all() and torch.equal(info["weight"], info2["weight"])
    for m in (1, b - 1):
        _, alone = _geo().hungarian_mean(_dev(a[m:m + 1]), anchor=anchor, max_sweeps=1)
        assert torch.equal(alone["perm"][0], info["perm"][m]) and torch.equal(alone["sign"][0], info["sign"][m])
        assert alone["cost"][0, 0] == info["cost"][0, m]
    Yc, ic = _geo().hungarian_mean(_dev(a))
    Yc2, ic2 = _geo().hungarian_mean(_dev(a))
    assert torch.equal(Yc, Yc2) and torch.equal(ic["perm"], ic2["perm"]) and ic["sweeps"] == ic2["sweeps"]
