"""geometry.flag_mean (dpb_flag_mean_init / _iterate / _finish, csrc/flagmean.hip) and frechet_mean(init="flag") on the GPU against tests/_flag_ref.py,
the numpy float64 reference in the ambient space (QR, one SVD of the stacked Q's, scipy's angles), on the same fp32 inputs.

Bars, the project's own for its geometry: for every j <= r with a relative gap >= 0.05 after row j in the reference's spectrum, the largest principal
angle between span Y[:j] and the reference's <= 1e-6 rad (the nesting with it); weight within 4 2^-24; Y Y^T within 4 2^-24 of I; theta within 1e-6 rad."""
import functools

import numpy as np
import pytest
import torch

import _flag_ref as R
import _frechet_ref as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 1e-6
EPS = 4 * 2.0 ** -24
GAP = 0.05
NOISE = {1: (0.1,), 3: (0.1, 0.45, 0.87), 4: (0.1, 0.3, 0.6, 0.9)}

# (kind, B, k, N, r): 'graded' for r < k, a clustered set of that spread for r = k
CASES = [("graded", 1, 1, 5, 1), (0.5, 2, 3, 64, 3), ("graded", 7, 5, 131, 3), (0.6, 7, 5, 131, 5), ("graded", 33, 2, 40, 1), ("graded", 5, 16, 517, 4),
         ("graded", 3, 64, 4099, 3), (1.0, 3, 64, 4099, 64), (0.2, 40, 32, 2050, 32)]


def _geo():
    from diffusion_pullback_amd import geometry
    return geometry


def _dev(a):
    return torch.tensor(np.asarray(a), device=DEV)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def _case(kind, b, k, n, r):
    rng = np.random.default_rng(100 * b + k + r)
    a = R.graded_set(rng, b, k, n, NOISE[r]) if kind == "graded" else R.clustered_set(rng, b, k, n, spread=kind)
    a.setflags(write=False)
    return a, R.flag_mean_ref(a, r)


def _check(a, r, Y, info, Yr, ir, what, need_converged=True):
    b, k, _ = a.shape
    Y = _np(Y)
    gaps = R.rel_gaps(ir["eigenvalues"])
    assert gaps[r - 1] >= GAP, f"{what}: the set has no gap after row {r}"
    rows = [j for j in range(1, r + 1) if gaps[j - 1] >= GAP]
    angs = [R.max_angle(Y[:j], Yr[:j]) for j in rows]
    w_err = np.abs(_np(info["weight"]) - ir["weight"]).max()
    orth = np.abs(Y @ Y.T - np.eye(r)).max()
    th_err = np.abs(_np(info["theta"]) - ir["theta"]).max()
    print(f"{what}: {info['iterations']} iterations, residual {info['residual']:.2e}, gap {info['gap']}; rows with a gap {rows}: angles "
          f"{['%.1e' % x for x in angs]}; weight {w_err:.2e} (bar {EPS:.2e}), |Y Y^T - I| {orth:.2e}, theta {th_err:.2e}")
    assert info["converged"] or not need_converged, what
    assert max(angs) <= BAR, what
    assert w_err <= EPS, what
    assert orth <= EPS, what
    assert th_err <= BAR, what
    assert tuple(info["theta"].shape) == (b, min(r, k)) and (np.diff(_np(info["theta"]), axis=1) <= 0).all(), what
    assert (np.diff(_np(info["weight"])) <= 0).all(), what
    m = R.block_width(b * k, r)
    assert len(info["eigenvalues"]) == m, what
    assert np.abs(info["eigenvalues"][:r] - ir["eigenvalues"][:r]).max() <= EPS, what
    assert (info["gap"] is None) == (m == r), what


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_flag_mean_matches_the_reference(case):
    kind, b, k, n, r = case
    a, (Yr, ir) = _case(*case)
    Y, info = _geo().flag_mean(_dev(a), rank=r)
    _check(a, r, Y, info, Yr, ir, f"{case}")
    if b == 1:
        assert R.max_angle(_np(Y), a[0]) <= BAR and abs(float(info["weight"][0]) - 1.0) <= EPS


def test_rank_none_is_k_and_two_runs_are_bitwise_equal():
    case = (0.6, 7, 5, 131, 5)
    a, (Yr, ir) = _case(*case)
    Y0, i0 = _geo().flag_mean(_dev(a))
    Y1, i1 = _geo().flag_mean(_dev(a), rank=5)
    assert tuple(Y0.shape) == (5, 131)
    assert torch.equal(Y0, Y1) and torch.equal(i0["weight"], i1["weight"]) and torch.equal(i0["theta"], i1["theta"])
    assert np.array_equal(i0["eigenvalues"], i1["eigenvalues"]) and i0["iterations"] == i1["iterations"] and i0["residual"] == i1["residual"]
    case = ("graded", 5, 16, 517, 4)
    a, _ = _case(*case)
    Y0, i0 = _geo().flag_mean(_dev(a), rank=4)
    Y1, i1 = _geo().flag_mean(_dev(a), rank=4)
    assert torch.equal(Y0, Y1) and torch.equal(i0["weight"], i1["weight"]) and np.array_equal(i0["eigenvalues"], i1["eigenvalues"])


def test_remixed_rows_give_the_same_spans():
    rng = np.random.default_rng(5)
    a = R.quantised(R.graded_set(rng, 6, 7, 300, NOISE[3], cond=1.0) * 0.5)
    Yr, ir = R.flag_mean_ref(a, 3)
    Ya, ia = _geo().flag_mean(_dev(a), rank=3)
    Yb, ib = _geo().flag_mean(_dev(R.remix(a)), rank=3)
    _check(a, 3, Ya, ia, Yr, ir, "quantised")
    _check(a, 3, Yb, ib, Yr, ir, "remixed")


def test_unconverged_run_still_returns_an_orthonormal_basis_with_its_rayleigh_quotients():
    a = R.spread_set(np.random.default_rng(6), b=6, k=6, n=2048)
    Y, info = _geo().flag_mean(_dev(a), rank=3, max_iter=8)
    Yn = _np(Y)
    w = R.rayleigh_weights(a, Yn)
    err = np.abs(_np(info["weight"]) - w).max()
    orth = np.abs(Yn @ Yn.T - np.eye(3)).max()
    print(f"spread set, 8 iterations: residual {info['residual']:.2e}, weight against mean ||Q y||^2 {err:.2e}, |Y Y^T - I| {orth:.2e}, "
          f"spectrum {np.round(info['eigenvalues'][:6], 4)}")
    assert not info["converged"] and info["iterations"] == 8
    assert orth <= EPS
    assert err <= 1e-6


def test_errors():
    g = _geo()
    a = np.array(_case(0.6, 7, 5, 131, 5)[0])
    for bad in (0, 36, 65):
        with pytest.raises(ValueError, match="rank"):
            g.flag_mean(_dev(a), rank=bad)
    with pytest.raises(ValueError, match="rank"):
        g.flag_mean(_dev(np.random.default_rng(0).standard_normal((4, 2, 3)).astype(np.float32)), rank=4)          # N = 3 < r
    with pytest.raises(ValueError, match="max_bytes"):
        g.flag_mean(_dev(a), max_bytes=1000)
    a[2, 1] = 0.0
    a[5, 3] = a[5, 0]
    with pytest.raises(ValueError, match=r"degenerate.*\[2, 5\]"):
        g.flag_mean(_dev(a), rank=2)
    Y, info = g.flag_mean(_dev(a), rank=2, check=False)
    assert info["degenerate"] == [2, 5] and not info["converged"]
    assert bool(torch.isnan(Y).all()) and bool(torch.isnan(info["weight"]).all()) and bool(torch.isnan(info["theta"]).all())
    with pytest.raises(ValueError, match="init"):
        g.frechet_mean(_dev(a), init="mean")
    with pytest.raises(ValueError, match="init"):
        g.frechet_mean(_dev(a), init=7)


def test_flag_start_reaches_a_mean_no_member_start_can():
    a = R.domain_set(np.random.default_rng(7))
    with pytest.raises(ValueError, match="domain"):
        _geo().frechet_mean(_dev(a), init=0)
    Yf, _ = R.flag_mean_ref(a)
    far = [R.max_angle(Yf, x) for x in a]
    Yr, steps, ok = R.karcher_from(a, Yf, tol=1e-10)
    Y, info = _geo().frechet_mean(_dev(a), init="flag", tol=1e-10)
    ang = R.max_angle(_np(Y), Yr)
    print(f"domain set: the flag mean lies {min(far):.2f} .. {max(far):.2f} rad from the members; {info['iterations']} Karcher steps from it (reference "
          f"{steps}), flag solver {info['flag_iterations']} iterations; angle to the reference's mean {ang:.2e}")
    assert ok and info["converged"] and info["flag_converged"]
    assert ang <= BAR


@functools.lru_cache(maxsize=None)
def _karcher_sets():
    """clustered sets on which, in the float64 reference, the flag start takes no more Karcher steps than member 0 (chosen on the CPU)"""
    keep = []
    for seed, (b, k, n, spread) in enumerate([(7, 5, 131, 0.3), (12, 6, 257, 0.6), (9, 17, 600, 1.0), (5, 3, 64, 0.8)]):
        a = R.clustered_set(np.random.default_rng(40 + seed), b, k, n, spread=spread)
        Y0, i0 = F.frechet_mean_ref(a, tol=1e-10)
        Y1, s1, ok = R.karcher_from(a, R.flag_mean_ref(a)[0], tol=1e-10)
        if i0["converged"] and ok and s1 <= i0["iterations"]:
            keep.append((a, Y0, i0["iterations"], s1))
    return keep


def test_flag_start_agrees_with_member_start_in_no_more_steps():
    sets = _karcher_sets()
    assert sets, "no clustered set kept: the reference itself does not show the property"
    for a, Yr, s0, s1 in sets:
        Ya, ia = _geo().frechet_mean(_dev(a), init=0, tol=1e-10)
        Yb, ib = _geo().frechet_mean(_dev(a), init="flag", tol=1e-10)
        ang = R.max_angle(_np(Ya), _np(Yb))
        print(f"B={a.shape[0]} k={a.shape[1]} N={a.shape[2]}: steps from member 0 {ia['iterations']} (reference {s0}), from the flag mean "
              f"{ib['iterations']} (reference {s1}); angle between the means {ang:.2e}, to the reference's {R.max_angle(_np(Yb), Yr):.2e}")
        assert ia["converged"] and ib["converged"]
        assert ang <= BAR
        assert ib["iterations"] <= ia["iterations"]
