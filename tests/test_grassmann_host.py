"""CPU-only: tests/_grassmann_ref.py (the textbook restatement the GPU tests of the Grassmann geodesics compare against) held to analytic two-plane
constructions and to scipy.linalg.subspace_angles, and the argument checks of the new entry points that fail before any device call."""
import os

import numpy as np
import pytest
import torch
from scipy.linalg import subspace_angles

import _grassmann_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS = [-0.5, 0.0, 0.25, 0.5, 1.0, 1.5]


def _two_planes(theta):
    """span{e0, e1} and span{cos t0 e0 + sin t0 e2, cos t1 e1 + sin t1 e3} in R^5: the geodesic rotates each e_i towards its partner"""
    e = np.eye(5)
    a = np.stack([e[0], e[1]])
    b = np.stack([np.cos(theta[0]) * e[0] + np.sin(theta[0]) * e[2], np.cos(theta[1]) * e[1] + np.sin(theta[1]) * e[3]])
    return e, a, b


@pytest.mark.parametrize("theta", [(1.0, 0.3), (1e-6, 1e-3), (np.pi / 2 - 1e-3, 0.5)])
def test_reference_against_the_analytic_two_plane_geodesic(theta):
    e, a, b = _two_planes(theta)
    mix = np.array([[2.0, 1.0], [-1.0, 3.0]])
    y = R.geodesic(mix @ a, mix.T @ b, TS)                           # a basis change moves no span
    for j, t in enumerate(TS):
        want = np.stack([np.cos(t * theta[0]) * e[0] + np.sin(t * theta[0]) * e[2], np.cos(t * theta[1]) * e[1] + np.sin(t * theta[1]) * e[3]])
        assert R.max_angle(y[j], want) <= 1e-12 * max(1.0, np.tan(max(theta)))
        assert np.abs(y[j] @ y[j].T - np.eye(2)).max() <= 1e-12
    op = R.log_operator(mix @ a, b)
    want = theta[0] * np.outer(e[2], e[0]) + theta[1] * np.outer(e[3], e[1])          # e0 -> theta0 e2, e1 -> theta1 e3
    assert np.abs(op - want).max() <= 1e-12 * max(1.0, np.tan(max(theta)))
    _, _, th, _ = R.tangent(a, b)
    assert np.abs(np.sort(th)[::-1] - np.sort(theta)[::-1]).max() <= 1e-12


def test_reference_exp_inverts_the_log_and_ignores_what_is_not_horizontal():
    theta = (0.9, 0.2)
    e, a, b = _two_planes(theta)
    h = np.stack([theta[0] * e[2], theta[1] * e[3]])
    y, s = R.exp_map(a, h, [1.0, 0.5])
    assert R.max_angle(y[0], b) <= 1e-14 and np.abs(s - np.array(theta)).max() <= 1e-14
    half = np.stack([np.cos(0.45) * e[0] + np.sin(0.45) * e[2], np.cos(0.1) * e[1] + np.sin(0.1) * e[3]])
    assert R.max_angle(y[1], half) <= 1e-14
    # P not orthonormal, H with a part inside span P: the tangent is p_i -> the horizontal part of h_i
    mix = np.array([[2.0, 1.0], [-1.0, 3.0]])
    y2, s2 = R.exp_map(mix @ a, mix @ h + np.array([[5.0, -2.0], [1.0, 4.0]]) @ a, [1.0])
    assert R.max_angle(y2[0], b) <= 1e-14 and np.abs(s2 - s).max() <= 1e-14
    assert np.abs(R.tangent_operator(mix @ a, mix @ h) - R.log_operator(a, b)).max() <= 1e-14


@pytest.mark.parametrize("k,n", [(1, 7), (5, 67), (17, 259), (64, 128)])
@pytest.mark.parametrize("name", ["tiny", "mixed", "spread", "random"])
def test_reference_angles_against_scipy_on_the_planted_inputs(k, n, name):
    rng = np.random.default_rng(k + n)
    for variant in range(3):
        a, b = R.family(rng, k, n, name, variant)
        _, _, th, _ = R.tangent(a, b)
        want = subspace_angles(a.astype(np.float64).T, b.astype(np.float64).T)
        assert np.abs(np.sort(th)[::-1] - want).max() <= 1e-9 * max(1.0, np.tan(want.max())) ** 2          # (theta = atan s: the error of s over 1 + s^2)
        y = R.geodesic(a, b, [0.0, 1.0])
        assert R.max_angle(y[0], a) <= 1e-9 and R.max_angle(y[1], b) <= 1e-9


def test_intersecting_pairs_stay_inside_the_domain():
    for k, n in [(5, 7), (16, 20), (64, 100)]:
        a, b = R.random_pair(k, n)
        th = R.angles_to(a, b)
        assert th[0] < np.pi / 2 - 1e-3 and (th[-(2 * k - n):] <= 1e-6).all()          # the spans share 2k - N directions


def _lib():
    from diffusion_pullback_amd import lib
    return lib, lib.load()


def test_symbols_are_exported_and_declared():
    lib, so = _lib()
    header = open(os.path.join(ROOT, "include", "dpb.h")).read()
    for name in ("dpb_grassmann_scratch_bytes", "dpb_grassmann_pair", "dpb_grassmann_exp"):
        assert name in lib.SYMBOLS and getattr(so, name) is not None and name in header, name
    assert so.dpb_abi_version() == 1


def test_scratch_bytes_is_zero_for_invalid_arguments():
    _, so = _lib()
    f = so.dpb_grassmann_scratch_bytes
    assert f(8, 9, 50, 196608) > 0 and f(1, 1, 1, 1) > 0 and f(65535, 64, 64, 64) > 0
    assert f(3, 1, 5, 67) == f(3, 2, 5, 67)                          # modes 0 and 1 write two slices
    for d, j, k, n in [(2, 6, 65, 128), (2, 6, 8, 7), (0, 6, 4, 16), (65536, 6, 4, 16), (2, 0, 4, 16), (2, 65, 4, 16), (2, 6, 0, 16), (2, 6, 4, 0)]:
        assert f(d, j, k, n) == 0, (d, j, k, n)


def test_arguments_are_checked_before_any_gpu_call():
    import ctypes as C
    lib, so = _lib()
    msg = lambda: so.dpb_last_error().decode()
    one = 256                                                        # any aligned non-null value: the checks below fail before a pointer is used
    ts = (C.c_double * 2)(0.0, 1.0)
    pair = lambda a=one, stride=4 * 64, d=2, k=4, n=64, mode=2, t=ts, j=2, o1=None, scr=one, sb=1 << 30: \
        so.dpb_grassmann_pair(a, stride, one, d, k, n, mode, t, j, one, o1, one, one, scr, sb, None)
    assert pair(a=None) != 0 and "null" in msg()
    assert pair(mode=0) != 0 and "null" in msg()                     # modes 0 and 1 need out1
    assert pair(mode=3) != 0 and "mode=3 outside [0,2]" in msg()
    assert pair(k=65, n=128, stride=65 * 128) != 0 and "k=65 outside [1,64]" in msg()
    assert pair(k=8, n=7, stride=56) != 0 and "N=7 < k" in msg()
    assert pair(stride=100) != 0 and "a_stride=100 must be 0" in msg()
    assert pair(t=None) != 0 and "ts is null" in msg()
    assert pair(j=65) != 0 and "J=65 outside [1,64]" in msg()
    assert pair(scr=one + 8) != 0 and "256-byte aligned" in msg()
    assert pair(sb=1024) != 0 and "dpb_grassmann_scratch_bytes(2, 2, 4, 64)" in msg()
    assert so.dpb_grassmann_exp(one, None, 2, 4, 64, ts, 2, one, one, one, one, 1 << 30, None) != 0 and "null" in msg()
    assert so.dpb_grassmann_exp(one, one, 2, 65, 128, ts, 2, one, one, one, one, 1 << 30, None) != 0 and "k=65 outside [1,64]" in msg()
    assert so.dpb_grassmann_exp(one, one, 2, 4, 64, ts, 2, one, one, one, one, 1024, None) != 0 and "scratch of 1024 bytes" in msg()


def test_there_is_no_cpu_fallback():
    from diffusion_pullback_amd import geometry, lib
    x = torch.zeros(2, 4, 64)
    for fn, extra in [(geometry.principal_vectors, ()), (geometry.grassmann_log, ()), (geometry.grassmann_geodesic, (0.5,)), (geometry.grassmann_exp, (0.5,))]:
        with pytest.raises(lib.DpbError, match="no CPU fallback"):
            fn(x, x, *extra)
    with pytest.raises(ValueError, match="1 .. 64 parameters"):
        geometry._times([])
    with pytest.raises(ValueError, match="1 .. 64 parameters"):
        geometry._times([0.0] * 65)
    assert geometry._times(0.5) == [0.5] and geometry._times((0, 1)) == [0.0, 1.0]


def test_module_docstring_and_readme_name_the_maps():
    from diffusion_pullback_amd import geometry
    assert "grassmann_exp" in geometry.__doc__ and "still no public exponential" not in geometry.__doc__
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "grassmann_geodesic" in readme
