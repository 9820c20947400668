"""geometry.flag_mean(weights=) and geometry.flag_median (dpb_flag_median_*, csrc/flagmean.hip) on the GPU against tests/_flag_median_ref.py, the numpy
float64 reference in the ambient space (QR, one SVD of the stacked sqrt(w_i) Q_i per round, scipy's angles), on the same fp32 inputs.

Bars, the flag mean's own: for every j <= r with a relative gap >= 0.05 after row j in the reference's spectrum, the largest principal angle between
span Y[:j] and the reference's <= 1e-6 rad; weight and Y Y^T - I within 4 2^-24; theta within 1e-6 rad.  The median, on the planted sets that meet the
conditions of _flag_median_ref.qualifies (asserted on the reference first): the same number of rounds, every round's objective within 1e-9 relative,
member_weight and distance within 1e-8 relative, the final span within 1e-6 rad."""
import functools

import numpy as np
import pytest
import torch

import _flag_median_ref as M
import _flag_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 1e-6
EPS = 4 * 2.0 ** -24
GAP = 0.05

# (B, k, N, r): one member; R = 15 odd and m = R (the scalar load path); R > N; member boundaries inside the 16-column chunks; several workgroups;
# k = r = 64
MEAN_CASES = [(1, 1, 5, 1), (3, 2, 9, 1), (5, 3, 67, 2), (7, 5, 33, 5), (20, 6, 200, 3), (9, 8, 130, 4), (40, 32, 2050, 10), (3, 64, 4099, 64)]


def _geo():
    from diffusion_pullback_amd import geometry
    return geometry


def _dev(a):
    return torch.tensor(np.asarray(a), device=DEV)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def _mean_set(b, k, n, r):
    rng = np.random.default_rng(1000 * b + 10 * k + r)
    a = R.clustered_set(rng, b, k, n, spread=0.6) if r == k else R.graded_set(rng, b, k, n, tuple(np.linspace(0.1, 0.8, r)))
    a.setflags(write=False)
    return a


def mean_weights(b, kind):
    """'decades': random positive weights over two decades; 'zeros': the same with about a third of them zero (never all)"""
    rng = np.random.default_rng(7 * b + 1)
    w = 10.0 ** rng.uniform(-1.0, 1.0, b)
    if kind == "zeros":
        w[rng.permutation(b)[:b // 3]] = 0.0
    return w


@functools.lru_cache(maxsize=None)
def _mean_case(b, k, n, r, kind):
    a = _mean_set(b, k, n, r)
    return a, mean_weights(b, kind), M.weighted_flag_mean_ref(a, r, mean_weights(b, kind))


@functools.lru_cache(maxsize=None)
def _planted(idx):
    (b_in, b_out, k, n, r), seed, shared = M.PLANTED[idx]
    a, frame = M.planted(np.random.default_rng(seed), b_in, b_out, k, n, r, out_shared=shared)
    a.setflags(write=False)
    return a, frame, M.flag_median_ref(a, r), M.weighted_flag_mean_ref(a, r)


def _check_basis(r, Y, info, Yr, ir, what):
    """the flag mean's bars on Y, weight, theta against a reference solve"""
    Y = _np(Y)
    gaps = R.rel_gaps(ir["eigenvalues"])
    assert gaps[r - 1] >= GAP, f"{what}: the set has no gap after row {r}"
    rows = [j for j in range(1, r + 1) if gaps[j - 1] >= GAP]
    angs = [R.max_angle(Y[:j], Yr[:j]) for j in rows]
    w_err = np.abs(_np(info["weight"]) - ir["weight"]).max()
    orth = np.abs(Y @ Y.T - np.eye(r)).max()
    th_err = np.abs(_np(info["theta"]) - ir["theta"]).max()
    print(f"{what}: rows with a gap {rows}: angles {['%.1e' % x for x in angs]}; weight {w_err:.2e} (bar {EPS:.2e}), |Y Y^T - I| {orth:.2e}, "
          f"theta {th_err:.2e}")
    assert max(angs) <= BAR, what
    assert w_err <= EPS, what
    assert orth <= EPS, what
    assert th_err <= BAR, what


@pytest.mark.parametrize("kind", ["decades", "zeros"])
@pytest.mark.parametrize("case", MEAN_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_weighted_mean_matches_the_reference(case, kind):
    b, k, n, r = case
    a, w, (Yr, ir) = _mean_case(*case, kind)
    Y, info = _geo().flag_mean(_dev(a), rank=r, weights=torch.tensor(w) if kind == "decades" else list(w))
    assert info["converged"], case
    _check_basis(r, Y, info, Yr, ir, f"{case} {kind}")
    assert tuple(info["theta"].shape) == (b, min(r, k)) and np.isfinite(_np(info["theta"])).all()
    mw, aff = _np(info["member_weight"]), _np(info["affinity"])
    print(f"  member_weight {np.abs(mw - ir['member_weight']).max():.2e}, affinity {np.abs(aff - ir['affinity']).max():.2e}")
    assert np.abs(mw - ir["member_weight"]).max() <= 1e-12 * ir["member_weight"].max()
    assert np.abs(aff - ir["affinity"]).max() <= 1e-9 * r


@pytest.mark.parametrize("case", [(20, 6, 200, 3), (5, 3, 67, 2)], ids=lambda c: "-".join(str(x) for x in c))
def test_uniform_weights_are_the_unweighted_call(case):
    b, k, n, r = case
    a = _dev(_mean_set(*case))
    Y0, i0 = _geo().flag_mean(a, r)
    Y1, i1 = _geo().flag_mean(a, r, weights=torch.ones(b))
    assert torch.equal(Y0, Y1) and torch.equal(i0["weight"], i1["weight"])
    assert np.array_equal(i0["eigenvalues"], i1["eigenvalues"]) and i0["iterations"] == i1["iterations"]
    th = (i0["theta"] - i1["theta"]).abs().max().item()
    print(f"{case}: uniform weights bitwise; theta {th:.2e}")
    assert th <= BAR
    Y2, i2 = _geo().flag_mean(a, r, weights=[3.0] * b)          # any constant: the table is 1 again
    assert torch.equal(Y0, Y2) and torch.equal(i0["weight"], i2["weight"])


@pytest.mark.parametrize("case", [(20, 6, 200, 3), (5, 3, 67, 2)], ids=lambda c: "-".join(str(x) for x in c))
def test_zero_weight_excludes_the_member(case):
    b, k, n, r = case
    a = _mean_set(*case)
    mask = np.ones(b, bool)
    mask[[1, b - 1]] = False
    Yr, ir = R.flag_mean_ref(a[mask], r)
    Ys, isub = _geo().flag_mean(_dev(a[mask]), r)
    Y, info = _geo().flag_mean(_dev(a), r, weights=mask.astype(np.float64))
    gaps = R.rel_gaps(ir["eigenvalues"])
    rows = [j for j in range(1, r + 1) if gaps[j - 1] >= GAP]
    assert r in rows
    angs = [R.max_angle(_np(Y)[:j], _np(Ys)[:j]) for j in rows]
    angr = [R.max_angle(_np(Y)[:j], Yr[:j]) for j in rows]
    w_err = (info["weight"] - isub["weight"]).abs().max().item()
    th = _np(info["theta"])
    print(f"{case}: 0/1 weights against the subset's mean: angles {['%.1e' % x for x in angs]} (reference {['%.1e' % x for x in angr]}), weight {w_err:.2e}")
    assert max(angs) <= BAR and max(angr) <= BAR and w_err <= EPS
    assert th.shape == (b, min(r, k)) and np.isfinite(th).all()
    assert np.abs(th[mask] - _np(isub["theta"])).max() <= BAR
    assert np.abs(th - np.stack([R.angles_to(Yr, R.orthonormal_rows(x)) for x in a])).max() <= BAR


def test_the_conditions_hold_on_the_reference():
    """every planted set but at most one must qualify, converge and descend in the reference before anything is claimed of the device"""
    ok = []
    for idx in range(len(M.PLANTED)):
        _, _, (_, ir), _ = _planted(idx)
        print(M.PLANTED[idx], "rounds", ir["rounds"], "min gap %.3f" % ir["gaps"].min(), "min d %.3g" % ir["dmin"].min())
        assert ir["converged"] and ir["monotone"]
        ok.append(M.qualifies(ir))
    assert sum(ok) >= 5


@pytest.mark.parametrize("idx", range(len(M.PLANTED)), ids=lambda i: "-".join(str(x) for x in M.PLANTED[i][0]))
def test_median_matches_the_reference(idx):
    (b_in, b_out, k, n, r), _, _ = M.PLANTED[idx]
    a, frame, (Yr, ir), _ = _planted(idx)
    assert M.qualifies(ir), "the case does not meet the conditions (every listed case does on the reference)"
    geo = _geo()
    Y, info = geo.flag_median(_dev(a), rank=r)
    J, Jr = info["objective"], ir["objective"]
    print(f"{M.PLANTED[idx][0]}: rounds {info['rounds']} (reference {ir['rounds']}), inner iterations {info['inner_iterations']}")
    assert info["inner_converged"]
    assert info["rounds"] == ir["rounds"] and len(J) == len(Jr)
    j_err = np.abs(J - Jr) / Jr
    mw_err = (np.abs(_np(info["member_weight"]) - ir["member_weight"]) / ir["member_weight"]).max()
    d_err = (np.abs(_np(info["distance"]) - ir["distance"]) / ir["distance"]).max()
    ang = R.max_angle(_np(Y), Yr)
    w_err = np.abs(_np(info["weight"]) - ir["weight"]).max()
    orth = np.abs(_np(Y) @ _np(Y).T - np.eye(r)).max()
    aff = geo.flag_affinity(_dev(a), Y[None])[:, 0]
    a_err = (info["affinity"] - aff).abs().max().item()
    print(f"  objective {j_err.max():.2e} (bar 1e-9), member_weight {mw_err:.2e}, distance {d_err:.2e} (bar 1e-8), span {ang:.2e} (bar 1e-6), "
          f"weight {w_err:.2e}, |Y Y^T - I| {orth:.2e} (bar {EPS:.2e}), affinity against flag_affinity {a_err:.2e} (bar {EPS * r:.2e})")
    assert j_err.max() <= 1e-9
    assert mw_err <= 1e-8 and d_err <= 1e-8
    assert ang <= BAR
    assert w_err <= EPS and orth <= EPS
    assert info["monotone"] and info["converged"]
    assert a_err <= EPS * r
    assert np.abs(_np(info["theta"]) - ir["theta"]).max() <= BAR


@pytest.mark.parametrize("idx", [i for i, p in enumerate(M.PLANTED) if p[2]], ids=lambda i: "-".join(str(x) for x in M.PLANTED[i][0]))
def test_median_is_robust_where_the_mean_is_not(idx):
    (b_in, b_out, k, n, r), _, _ = M.PLANTED[idx]
    a, frame, (Yr, ir), (Ymr, _) = _planted(idx)
    ref_mean, ref_med = R.max_angle(Ymr, frame), R.max_angle(Yr, frame)
    assert ref_med < 0.5 * ref_mean, "the reference itself"
    assert ir["member_weight"][:b_in].min() > ir["member_weight"][b_in:].max(), "the reference itself"
    Ym, _ = _geo().flag_mean(_dev(a), rank=r)
    Y, info = _geo().flag_median(_dev(a), rank=r)
    dev_mean, dev_med = R.max_angle(_np(Ym), frame), R.max_angle(_np(Y), frame)
    w = _np(info["member_weight"])
    print(f"{M.PLANTED[idx][0]}: angle to the planted frame, mean {dev_mean:.3f} -> median {dev_med:.3f} (reference {ref_mean:.3f} -> {ref_med:.3f}); "
          f"weights: inliers >= {w[:b_in].min():.3f}, outliers <= {w[b_in:].max():.3f}")
    assert dev_med < 0.5 * dev_mean
    assert w[:b_in].min() > w[b_in:].max()


def test_two_runs_are_bitwise_equal_and_no_round_is_the_mean():
    a, _, _, _ = _planted(0)
    geo = _geo()
    Y0, i0 = geo.flag_median(_dev(a), rank=3)
    Y1, i1 = geo.flag_median(_dev(a), rank=3)
    assert torch.equal(Y0, Y1) and np.array_equal(i0["objective"], i1["objective"]) and i0["inner_iterations"] == i1["inner_iterations"]
    for key in ("member_weight", "distance", "affinity", "weight", "theta"):
        assert torch.equal(i0[key], i1[key]), key
    Ym, im = geo.flag_mean(_dev(a), rank=3, max_iter=200)
    Yz, iz = geo.flag_median(_dev(a), rank=3, max_rounds=0)
    assert iz["rounds"] == 0 and not iz["converged"] and len(iz["objective"]) == 1
    assert torch.equal(Ym, Yz) and torch.equal(im["weight"], iz["weight"])
    assert torch.equal(iz["member_weight"], torch.ones(len(a), dtype=torch.float64, device=DEV))
    w = mean_weights(len(a), "decades")
    Yw, iw = geo.flag_mean(_dev(a), rank=3, max_iter=200, weights=w)
    Yp, ip = geo.flag_median(_dev(a), rank=3, max_rounds=0, weights=w)
    assert torch.equal(Yw, Yp) and torch.equal(iw["member_weight"], ip["member_weight"])
    d = np.sqrt(np.maximum(3 - _np(ip["affinity"]), 0))
    assert abs(ip["objective"][0] - np.sum(_np(ip["member_weight"]) * d)) <= 1e-12 * ip["objective"][0]


def test_one_member_is_its_own_median():
    a = R.clustered_set(np.random.default_rng(3), 1, 3, 40, spread=0.5)
    Y, info = _geo().flag_median(_dev(a), rank=3)
    d, w = _np(info["distance"]), _np(info["member_weight"])
    print(f"B = 1: distance {d}, member_weight {w}, objective {info['objective']}, rounds {info['rounds']}")
    assert R.max_angle(_np(Y), a[0]) <= BAR
    assert d[0] <= 1e-5 and np.isfinite(w).all() and w[0] == 1.0
    assert info["converged"] and abs(info["objective"][-1] - 0.5e-5) <= 1e-4 * 0.5e-5      # phi(d) = eps / 2 + d^2 / (2 eps), d^2 <= 3 * 64 * 2^-52


def test_degenerate_members_and_bad_arguments():
    geo = _geo()
    a = np.array(_planted(0)[0])
    a[4, 2] = 0.0
    with pytest.raises(ValueError, match=r"indices \[4\]"):
        geo.flag_median(_dev(a), rank=3)
    Y, info = geo.flag_median(_dev(a), rank=3, check=False)
    assert info["degenerate"] == [4] and bool(torch.isnan(Y).all())
    with pytest.raises(ValueError, match=r"indices \[4\]"):
        geo.flag_mean(_dev(a), rank=3, weights=np.ones(len(a)))
    Y, info = geo.flag_mean(_dev(a), rank=3, weights=np.ones(len(a)), check=False)
    assert info["degenerate"] == [4] and bool(torch.isnan(Y).all())
    a = _dev(_planted(0)[0])
    with pytest.raises(ValueError, match="rank = 7 outside"):
        geo.flag_median(a, rank=7)
    with pytest.raises(ValueError, match="eps"):
        geo.flag_median(a, rank=3, eps=0.0)
    w = np.ones(20)
    w[[2, 5]] = [-1.0, np.inf]
    with pytest.raises(ValueError, match=r"indices \[2, 5\]"):
        geo.flag_median(a, rank=3, weights=w)
    with pytest.raises(ValueError, match=r"indices \[2, 5\]"):
        geo.flag_mean(a, rank=3, weights=torch.tensor(w))
    with pytest.raises(ValueError, match="positive sum"):
        geo.flag_mean(a, rank=3, weights=np.zeros(20))
    with pytest.raises(ValueError, match="one value per basis"):
        geo.flag_mean(a, rank=3, weights=np.ones(19))
