"""geometry.grassmann_pga on the GPU against tests/_pga_ref.py, the float64 ambient-space restatement (QR, SVD log maps, one SVD of the flattened tangents,
numpy lstsq), on the same fp32 inputs.  The reference takes its logs at the device's returned Y (made exactly orthonormal by its polar factor), so only
the analysis is under test; that Y spans what was asked for is checked on its own.

Bars: the 1e-6 of the geometry family -- tangent_gram per entry 1e-6 max|T|; variance and total_variance 1e-6 total_variance; scores and residual
1e-6 max|scores|; modes, slopes, intercept and the mean tangent as operators 1e-6 relative (the measure of tests/test_gpu_grassmann.py's log-map test);
modes[m] Y^T and the Gram of the flattened modes against the identity 4 * 2^-24; theta 1e-6 rad; r2 1e-6.  Every case first proves on the CPU that it is
a fair one: largest angle to the base below pi/2 - 1e-3 and a relative gap of at least 0.05 after each claimed mode.

Worst values seen on an MI355X are recorded in the README paragraph."""
import functools

import numpy as np
import pytest
import torch

import _frechet_ref as F
import _pga_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BAR = 1e-6
ORTH = 4 * 2.0 ** -24
# (B, k, N, M, base, noise, covariates P)
CASES = [(2, 1, 5, 1, "tensor", 0.0, 0), (6, 3, 40, 2, "frechet", 0.0, 1), (12, 8, 300, 3, "flag", 0.0, 2), (33, 16, 1030, 4, "tensor", 2e-2, 1),
         (40, 32, 1030, 6, "member", 0.0, 0), (5, 64, 4099, 2, "frechet", 0.0, 0), (130, 2, 50, 3, "tensor", 0.0, 1), (300, 1, 64, 3, "flag", 1e-2, 0),
         (1024, 1, 64, 3, "tensor", 1e-2, 1)]
IDS = [f"B{c[0]}-k{c[1]}-N{c[2]}-M{c[3]}-{c[4]}" for c in CASES]


@pytest.fixture(autouse=True)
def _one_blas_thread():
    """the host reference is hundreds of small QR / SVD calls: a threaded BLAS spends them waiting for its own pool"""
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        yield
        return
    with threadpool_limits(1):
        yield


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else t


def _pga(a, base, **kw):
    from diffusion_pullback_amd import geometry
    if isinstance(base, np.ndarray):
        base = torch.tensor(base.astype(np.float32), device=DEV)
    y, modes, info = geometry.grassmann_pga(torch.tensor(a, device=DEV), base=base, **kw)
    return _np(y), _np(modes), {key: _np(v) for key, v in info.items()}


@functools.lru_cache(maxsize=None)
def _set(b, k, n, m, noise, npar):
    rng = np.random.default_rng(1000 + 7 * b + k)
    x = None
    if npar:
        x = np.stack([np.linspace(0.1, 0.9, b), np.cos(np.arange(b) * 1.3)][:npar], axis=1)
    a, y0, d, c = R.planted_set(rng, b, k, n, m, noise=noise, covariate=None if x is None else x[:, 0])
    return a, y0, x


def _base_arg(kind, y0):
    return {"tensor": y0, "member": 0}.get(kind, kind)


@functools.lru_cache(maxsize=None)
def _run(case):
    b, k, n, m, kind, noise, npar = case
    a, y0, x = _set(b, k, n, m, noise, npar)
    kw = {"tol": 1e-2} if kind == "frechet" else {}
    y, modes, info = _pga(a, _base_arg(kind, y0), n_modes=m, covariates=x, **kw)
    ref = R.pga_ref(a, R.polar_rows(y), m, covariates=x)
    return a, y0, x, y, modes, info, ref


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_against_the_ambient_reference(case):
    b, k, n, m, kind, noise, npar = case
    a, y0, x, y, modes, info, ref = _run(case)
    gaps = R.relative_gaps(ref["spectrum"], m)
    print(f"{case}: largest angle to the base {ref['theta'].max():.3f}, relative gaps {np.round(gaps, 3)}, solver {info['solver']}")
    assert ref["theta"].max() < np.pi / 2 - 1e-3 and gaps.min() >= 0.05           # a fair case: inside the log map's domain, modes separated
    assert info["solver"] == ("jacobi" if b <= 128 else "subspace") and not info["degenerate"] and not info["domain"]
    # the base: the span asked for
    if kind == "tensor":
        assert F.max_angle(y, y0) <= BAR
    elif kind == "member":
        assert F.max_angle(y, a[0]) <= BAR
    y64 = R.polar_rows(y)
    tmax, total, smax = np.abs(ref["tangent_gram"]).max(), ref["total_variance"], np.abs(ref["scores"]).max()
    worst = {"gram": np.abs(info["tangent_gram"] - ref["tangent_gram"]).max() / tmax,
             "variance": np.abs(info["variance"] - ref["variance"]).max() / total, "total": abs(info["total_variance"] - total) / total,
             "explained": np.abs(info["explained"] - ref["explained"]).max(),
             "scores": np.abs(info["scores"] - ref["scores"]).max() / smax, "residual": np.abs(info["residual"] - ref["residual"]).max() / smax,
             "mean_norm": abs(info["mean_tangent_norm"] - ref["mean_tangent_norm"]) / max(smax, 1e-300),
             "theta": np.abs(info["theta"] - ref["theta"]).max(),
             "modes_op": max(R.operator_gap(y, modes[j], y64, ref["modes"][j]) for j in range(m)),
             "mean_op": R.operator_gap(y, info["mean_tangent"], y64, ref["mean_tangent"]) * ref["mean_tangent_norm"] / np.sqrt(tmax),
             "modes_y": np.abs(modes.astype(np.float64) @ y.astype(np.float64).T).max(),
             "modes_gram": np.abs(modes.reshape(m, -1).astype(np.float64) @ modes.reshape(m, -1).astype(np.float64).T - np.eye(m)).max()}
    if npar:
        worst["r2"] = abs(info["r2"] - ref["r2"])
        worst["slope_norm"] = np.abs(info["slope_norm"] - ref["slope_norm"]).max() / np.abs(ref["slope_norm"]).max()
        worst["slopes_op"] = max(R.operator_gap(y, info["slopes"][p], y64, ref["slopes"][p]) for p in range(npar))
        worst["intercept_op"] = R.operator_gap(y, info["intercept"], y64, ref["intercept"]) * np.linalg.norm(ref["intercept"]) / np.sqrt(tmax)
    print("   worst:", {key: float(f"{v:.2e}") for key, v in worst.items()})
    for key, v in worst.items():
        assert v <= (ORTH if key in ("modes_y", "modes_gram") else BAR), (key, v)
    assert (np.diff(info["variance"]) <= 0).all() and (np.diff(info["theta"], axis=1) <= 0).all()
    for j in range(m):                                                            # the sign rule
        i = int(np.argmax(np.abs(ref["scores"][:, j])))
        assert info["scores"][i, j] > 0


def test_frechet_base_returns_the_bits_of_frechet_mean():
    """tol = 1e-2: the mean tangent norm sqrt(1^T T 1) / B is a sum that cancels down to the gradient; at g ~ 1e-3 and entries of T ~ 1e-1 the fp64 sum
    keeps 1e-12 relative, inside the 1e-9 asked for -- at the default tol the gradient is 1e-7 and its square is below the rounding of the sum"""
    from diffusion_pullback_amd import geometry
    case = CASES[1]
    a, y0, x, y, modes, info, ref = _run(case)
    ym, minfo = geometry.frechet_mean(torch.tensor(a, device=DEV), tol=1e-2)
    assert np.array_equal(_np(ym), y) and minfo["converged"] and info["converged"] and info["iterations"] == minfo["iterations"]
    rel = abs(info["mean_tangent_norm"] - minfo["grad_norm"]) / minfo["grad_norm"]
    print(f"mean_tangent_norm {info['mean_tangent_norm']!r} against grad_norm {minfo['grad_norm']!r}: relative {rel:.2e}")
    assert rel <= 1e-9
    a, y0, x, y, modes, info, ref = _run(CASES[2])                                # the flag base: the start of frechet_mean(init="flag"), no step
    yf, finfo = geometry.frechet_mean(torch.tensor(a, device=DEV), init="flag", max_iter=0)
    assert np.array_equal(_np(yf), y) and info["iterations"] == 0


@pytest.mark.parametrize("case", [CASES[2], CASES[4]], ids=[IDS[2], IDS[4]])
def test_round_trip_rebuilds_every_member_up_to_its_residual(case):
    from diffusion_pullback_amd import geometry
    b, k, n, m, kind, noise, npar = case
    a, y0, x, y, modes, info, ref = _run(case)
    yt = torch.tensor(y, device=DEV)
    worst = 0.0
    for i in range(b):
        h = info["mean_tangent"].astype(np.float64) + np.tensordot(info["scores"][i], modes.astype(np.float64), axes=1)
        z, _ = geometry.grassmann_exp(yt, torch.tensor(h.astype(np.float32), device=DEV), 1.0)
        ang = F.max_angle(_np(z)[0, 0], a[i])
        worst = max(worst, ang - info["residual"][i])
        assert ang <= info["residual"][i] + BAR, (i, ang, info["residual"][i])
    print(f"{case}: largest (angle to the member - residual) {worst:.2e}")


def test_prediction_at_a_held_out_covariate():
    from diffusion_pullback_amd import geometry
    b, k, n = 9, 4, 200
    x = np.linspace(-1.0, 1.0, b + 1) ** 3 + np.linspace(0.0, 0.5, b + 1)
    a, y0, d, c = R.planted_set(np.random.default_rng(5), b + 1, k, n, 1, covariate=x)
    y, modes, info = _pga(a[:b], y0, n_modes=1, covariates=x[:b])
    h = info["intercept"] + x[b] * info["slopes"][0]
    z, _ = geometry.grassmann_exp(torch.tensor(y, device=DEV), torch.tensor(h, device=DEV), 1.0)
    ang = F.max_angle(_np(z)[0, 0], a[b])
    print(f"prediction at the held-out covariate: {ang:.2e} rad, r2 {info['r2']!r}")
    assert ang <= BAR and abs(info["r2"] - 1.0) <= BAR


def test_two_runs_are_bitwise_equal():
    for case in (CASES[3], CASES[6]):
        b, k, n, m, kind, noise, npar = case
        a, y0, x, y, modes, info, ref = _run(case)
        y2, modes2, info2 = _pga(a, _base_arg(kind, y0), n_modes=m, covariates=x)
        assert np.array_equal(y, y2) and np.array_equal(modes, modes2)
        for key in ("variance", "scores", "residual", "tangent_gram", "theta", "mean_tangent", "slopes", "intercept"):
            assert np.array_equal(info[key], info2[key]), key
        assert info["r2"] == info2["r2"] and info["total_variance"] == info2["total_variance"]


def test_members_equal_to_the_base_give_zeros():
    """copies of one basis (scaled by powers of two: the same spans exactly): sin^2 theta is a difference of O(1) fp64 quantities, so the angles are
    rounding, below 1e-7, and every statistic is zero to 1e-12 -- and none is NaN"""
    rng = np.random.default_rng(9)
    one = F.clustered_set(rng, 1, 5, 120)[0]
    a = np.stack([one * 2.0 ** (i % 3) for i in range(7)])
    for base in (0, one.astype(np.float64), "frechet"):
        y, modes, info = _pga(a, base, n_modes=3)
        for key in ("variance", "explained", "scores", "residual", "tangent_gram", "theta"):
            assert np.isfinite(info[key]).all(), key
        assert np.isfinite(modes).all() and np.isfinite(y).all()
        assert np.abs(info["variance"]).max() <= 1e-12 and info["total_variance"] <= 1e-12 and np.abs(info["scores"]).max() <= 1e-6
        assert (info["explained"] == 0).all() and np.abs(info["tangent_gram"]).max() <= 1e-12 and np.abs(info["theta"]).max() <= 1e-6
        assert (modes == 0).all()


def _spoiled():
    a, y0, _ = _set(12, 8, 300, 3, 0.0, 2)
    a = a.copy()
    away = F.orthonormal_rows(np.concatenate([y0, np.random.default_rng(3).standard_normal((1, 300))]))[-1]      # a unit vector orthogonal to span Y0
    far = y0.copy()
    far[0] = away                                                                  # one direction at pi/2 from the base
    return a, y0, far.astype(np.float32)


def test_invalid_members_are_named_and_spoil_only_their_own_row_and_column():
    a, y0, far = _spoiled()
    at, az = a.copy(), a.copy()
    at[2] = far
    az[4, 1] = 0.0
    with pytest.raises(ValueError, match=r"outside the log map's domain.*pi/2 - 1e-6.*indices \[2\]"):
        _pga(at, y0, n_modes=3)
    with pytest.raises(ValueError, match=r"degenerate bases.*indices \[4\]"):
        _pga(az, y0, n_modes=3)
    both = at.copy()
    both[4, 1] = 0.0
    for label, arr, out in (("domain", at, [2]), ("degenerate", az, [4]), ("both", both, [2, 4])):
        y, modes, info = _pga(arr, y0, n_modes=3, check=False)
        keep = [i for i in range(len(arr)) if i not in out]
        t, s = info["tangent_gram"], info["scores"]
        nan_t = np.isnan(t)
        want = np.zeros_like(nan_t)
        want[out, :] = True
        want[:, out] = True
        assert np.array_equal(nan_t, want), label
        assert np.array_equal(np.isnan(s), np.repeat(np.isin(np.arange(len(arr)), out)[:, None], 3, axis=1)), label
        assert np.array_equal(np.isnan(info["residual"]), np.isin(np.arange(len(arr)), out)), label
        assert info["domain"] == [i for i in out if i == 2] and info["degenerate"] == [i for i in out if i == 4]
        ref = R.pga_ref(arr[keep], y0, 3)                                          # the statistics are those of the others (a rotation of Y's rows moves none)
        tmax, total, smax = np.abs(ref["tangent_gram"]).max(), ref["total_variance"], np.abs(ref["scores"]).max()
        assert np.abs(t[np.ix_(keep, keep)] - ref["tangent_gram"]).max() <= BAR * tmax, label
        assert np.abs(info["variance"] - ref["variance"]).max() <= BAR * total and abs(info["total_variance"] - total) <= BAR * total, label
        assert np.abs(s[keep] - ref["scores"]).max() <= BAR * smax, label
        if label == "domain":                                                      # no degenerate member: Y and the modes are numbers, and the right ones
            assert np.isfinite(modes).all() and F.max_angle(y, y0) <= BAR
            ref = R.pga_ref(arr[keep], R.polar_rows(y), 3)
            assert max(R.operator_gap(y, modes[j], R.polar_rows(y), ref["modes"][j]) for j in range(3)) <= BAR


@pytest.mark.parametrize("case", [CASES[3], CASES[4]], ids=[IDS[3], IDS[4]])
def test_both_eigen_routes_agree(case):
    from diffusion_pullback_amd import lib
    b, k, n, m, kind, noise, npar = case
    a, y0, x, y, modes, info, ref = _run(case)
    so = lib.load()
    assert so.dpb_debug_set(b"pga_route", 2) == 0
    try:
        y2, modes2, info2 = _pga(a, _base_arg(kind, y0), n_modes=m, covariates=x)
    finally:
        assert so.dpb_debug_set(b"pga_route", 0) == 0
    assert info["solver"] == "jacobi" and info2["solver"] == "subspace" and info2["subspace_converged"]
    assert np.array_equal(y, y2) and np.array_equal(info["tangent_gram"], info2["tangent_gram"])
    total, smax = ref["total_variance"], np.abs(ref["scores"]).max()
    y64 = R.polar_rows(y)
    worst = {"variance": np.abs(info["variance"] - info2["variance"]).max() / total, "scores": np.abs(info["scores"] - info2["scores"]).max() / smax,
             "residual": np.abs(info["residual"] - info2["residual"]).max() / smax,
             "modes_op": max(R.operator_gap(y, modes2[j], y64, ref["modes"][j]) for j in range(m))}
    print(f"{case}: the two routes differ by", {key: float(f"{v:.2e}") for key, v in worst.items()}, "subspace iterations", info2["subspace_iterations"])
    for key, v in worst.items():
        assert v <= BAR, (key, v)


def test_argument_errors():
    from diffusion_pullback_amd import geometry, lib
    a = torch.tensor(_set(6, 3, 40, 2, 0.0, 1)[0], device=DEV)
    with pytest.raises(lib.DpbError, match="HIP device"):
        geometry.grassmann_pga(a.cpu())
    with pytest.raises(ValueError, match="n_modes = 6 outside"):
        geometry.grassmann_pga(a, n_modes=6)
    with pytest.raises(ValueError, match="at least 2 members"):
        geometry.grassmann_pga(a[:1])
    with pytest.raises(ValueError, match="exceeds the rank 64"):
        geometry.grassmann_pga(torch.zeros(2, 65, 128, device=DEV))
    with pytest.raises(ValueError, match="exceeds their length"):
        geometry.grassmann_pga(torch.zeros(2, 8, 7, device=DEV))
    with pytest.raises(ValueError, match="max_bytes is 1000"):
        geometry.grassmann_pga(a, max_bytes=1000)
    with pytest.raises(ValueError, match="covariates must be"):
        geometry.grassmann_pga(a, covariates=[1.0, 2.0])
    with pytest.raises(ValueError, match="covariates must be finite"):
        geometry.grassmann_pga(a, covariates=[1.0, 2.0, float("nan"), 4.0, 5.0, 6.0])
    with pytest.raises(ValueError, match="rank 0 < P = 1"):
        geometry.grassmann_pga(a, covariates=[2.0] * 6)
    with pytest.raises(ValueError, match="base must be"):
        geometry.grassmann_pga(a, base="median")
    with pytest.raises(ValueError, match=r"base = 6 outside"):
        geometry.grassmann_pga(a, base=6)
    y, modes, info = geometry.grassmann_pga(a, base=1, center=False, n_modes=6)   # uncentred: up to B modes
    assert modes.shape == (6, 3, 40) and info["scores"].shape == (6, 6)
