"""CPU checks of principal geodesic analysis: tests/_pga_ref.py -- the float64 ambient-space restatement the GPU tests measure against -- is held to planted
sets whose answer is known; the k x k identity the pair kernel evaluates is held to the ambient Gram; then the sizer and the argument checks of the new
entry points, which run before any GPU call."""
import os

import numpy as np
import pytest
import torch

import _frechet_ref as F
import _grassmann_ref as G
import _pga_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-6


@pytest.mark.parametrize("b,k,n,m", [(6, 3, 40, 2), (12, 8, 300, 3), (9, 1, 30, 3)])
def test_planted_modes_are_recovered_at_the_planted_base(b, k, n, m):
    a, y0, d, c = R.planted_set(np.random.default_rng(b), b, k, n, m)
    r = R.pga_ref(a, y0, m)
    ev = np.linalg.eigvalsh(r["tangent_gram"])[::-1]
    print(f"B={b} k={k}: eigenvalues of T {ev[:m + 2]}, largest angle {r['theta'].max():.3f}")
    assert ev[m - 1] > 1e-3 and ev[m] <= 1e-10 * ev[0]                          # rank(T) = M (the members are rounded to fp32: 1e-7 relative, squared)
    dm, mm = d.reshape(m, -1), r["modes"].reshape(m, -1)
    assert np.linalg.svd(dm @ mm.T, compute_uv=False).min() >= 1 - 1e-9          # the span of the modes is the span of the D_m
    assert abs(r["spectrum"].sum() - r["total_variance"]) <= 1e-12 * r["total_variance"]
    assert np.abs(r["scores"] - (c - c.mean(axis=0)) @ (dm @ mm.T)).max() <= BAR  # the scores are the planted coefficients, in the modes' frame
    assert np.abs(r["logs"] @ y0.T).max() <= 1e-12 and r["residual"].max() <= BAR
    for j in range(m):
        assert r["scores"][np.argmax(np.abs(r["scores"][:, j])), j] > 0


def test_a_covariate_driven_set_is_explained_by_its_slope():
    b = 10
    x = np.linspace(0.0, 1.0, b) ** 2
    a, y0, d, c = R.planted_set(np.random.default_rng(1), b, 4, 100, 1, covariate=x)
    r = R.pga_ref(a, y0, 1, covariates=x)
    s = r["slopes"][0]
    cos = abs(np.sum(s * d[0])) / np.linalg.norm(s)
    print(f"r2 {r['r2']!r}, cosine of the slope to D_1 {cos!r}")
    assert abs(r["r2"] - 1) <= BAR and 1 - cos <= 1e-9
    assert abs(r["slope_norm"][0] - np.linalg.norm(s)) <= 1e-12
    pred = F.exp_map(y0, r["intercept"] + 0.37 * s)                             # the prediction lies on the planted geodesic
    t = np.polyfit(x, c[:, 0], 1)
    assert F.max_angle(pred, F.exp_map(y0, (t[1] + 0.37 * t[0]) * d[0])) <= BAR


def test_copies_of_one_basis_give_zeros():
    one = F.clustered_set(np.random.default_rng(2), 1, 5, 120)[0]
    a = np.stack([one * 2.0 ** i for i in range(4)])
    r = R.pga_ref(a, F.orthonormal_rows(one), 2)
    assert r["total_variance"] <= 1e-24 and np.abs(r["scores"]).max() <= 1e-12 and np.abs(r["variance"]).max() <= 1e-24
    assert np.isfinite(r["explained"]).all() and np.abs(r["tangent_gram"]).max() <= 1e-24 and r["residual"].max() <= 1e-12


@pytest.mark.parametrize("b,k,n", [(2, 1, 5), (6, 3, 40), (12, 8, 300), (7, 16, 20), (5, 33, 257)])
def test_the_k_by_k_identity_is_the_ambient_tangent_gram(b, k, n):
    rng = np.random.default_rng(10 * b + k)
    a = F.clustered_set(rng, b, k, n, spread=0.6)
    y = F.orthonormal_rows(np.mean(a.astype(np.float64), axis=0) + 0.1 * rng.standard_normal((k, n)) / np.sqrt(n))      # a base outside the members' span
    logs, _ = R.logs_at(y, a)
    flat = logs.reshape(b, -1)
    t = flat @ flat.T
    err = np.abs(R.tangent_gram_identity(a, y) - t).max() / np.abs(t).max()
    print(f"B={b} k={k} N={n}: identity against the ambient Gram {err:.2e} relative")
    assert err <= 1e-12


def test_operator_gap_is_the_norm_of_the_operator_difference():
    rng = np.random.default_rng(4)
    p1, p2 = rng.standard_normal((3, 20)), rng.standard_normal((3, 20))
    h1, h2 = rng.standard_normal((3, 20)), rng.standard_normal((3, 20))
    o1, o2 = G.tangent_operator(p1, h1), G.tangent_operator(p2, h2)
    assert abs(R.operator_gap(p1, h1, p2, h2) - np.linalg.norm(o1 - o2) / np.linalg.norm(o2)) <= 1e-12
    assert R.operator_gap(p1, h1, rng.standard_normal((3, 3)) @ p1, h1) >= 0.1       # (the operator depends on which row maps to which)
    m = rng.standard_normal((3, 3))
    assert R.operator_gap(m @ p1, m @ h1, p1, h1) <= 1e-7                             # ... and not on the basis the pair is written in


def test_cli_flags_parse(capsys):
    from diffusion_pullback_amd import main as m
    from diffusion_pullback_amd.edit import EditStableDiffusion, EditUncondDiffusion
    a = m.parse_args(["--note", "t"])
    assert a.run_tangent_space_pga is False and a.pga_base == "frechet" and a.pga_modes == 0
    a = m.parse_args(["--note", "t", "--run_tangent_space_pga", "True", "--pga_base", "flag", "--pga_modes", "3", "--distance_space", "h", "--h_t_list",
                      "0.8,0.5", "--num_local_basis", "4"])
    assert a.run_tangent_space_pga is True and (a.pga_base, a.pga_modes, a.distance_space) == ("flag", 3, "h")
    for bad in (["--pga_base", "median"], ["--pga_modes", "8", "--num_local_basis", "4", "--h_t_list", "0.8,0.5"], ["--num_local_basis", "1"]):
        with pytest.raises(SystemExit):
            m.parse_args(["--note", "t", "--run_tangent_space_pga", "True", *bad])
    capsys.readouterr()
    for flag in ("--run_tangent_space_pga", "--pga_base", "--pga_modes"):
        assert flag in m.__doc__
    for cls in (EditStableDiffusion, EditUncondDiffusion):                       # the job is on both drivers
        assert callable(getattr(cls, "run_tangent_space_pga"))


# ------------------------------------------------------------------------------------------------------------ the entry points
def _lib():
    from diffusion_pullback_amd import lib
    return lib, lib.load()


def test_symbols_are_exported_and_declared():
    lib, so = _lib()
    header = open(os.path.join(ROOT, "include", "dpb.h")).read()
    for name in ("dpb_pga_scratch_bytes", "dpb_pga_tangent_gram", "dpb_pga_eig", "dpb_pga_combine"):
        assert name in lib.SYMBOLS and getattr(so, name) is not None and name in header, name
    assert so.dpb_abi_version() == 1


def test_scratch_bytes_is_zero_for_invalid_arguments():
    _, so = _lib()
    f = so.dpb_pga_scratch_bytes
    assert f(3, 3, 5, 4096, 4) > 0 and f(4, 3, 5, 4096, 4) > f(3, 3, 5, 4096, 4) and f(1025, 1024, 1, 64, 80) > 8 * 1024 * 1024
    assert f(100, 100, 50, 196608, 18) > 8 * 5000 * 900                         # the coefficient matrices of 18 x 50 output rows
    assert f(3, 3, 5, 4096, 8) > f(3, 3, 5, 4096, 4)
    for b, m, k, n, j in [(0, 0, 4, 16, 2), (3, 1, 4, 16, 2), (3, 4, 4, 16, 2), (3, 3, 0, 16, 2), (3, 3, 65, 128, 2), (3, 3, 8, 7, 2), (3, 3, 4, 16, 0),
                          (3, 3, 4, 16, 81), (65536, 65536, 1, 16, 2)]:
        assert f(b, m, k, n, j) == 0, (b, m, k, n, j)


def test_arguments_are_checked_before_any_gpu_call():
    lib, so = _lib()
    msg = lambda: so.dpb_last_error().decode()
    one, big = 256, 1 << 40                                                     # any aligned non-null value: the checks below fail before a pointer is used
    assert so.dpb_pga_tangent_gram(3, 3, 4, 64, 10, 2, None, big, one, one, one, one, big, None) != 0 and "null" in msg()
    assert so.dpb_pga_tangent_gram(3, 3, 65, 128, 10, 2, one, big, one, one, one, one, big, None) != 0 and "no Frechet problem" in msg()
    assert so.dpb_pga_tangent_gram(3, 1, 4, 64, 10, 2, one, big, one, one, one, one, big, None) != 0 and "members=1 outside" in msg()
    assert so.dpb_pga_tangent_gram(3, 3, 4, 64, 10, 2, one, big, one, one, one, one + 8, big, None) != 0 and "256-byte aligned" in msg()
    assert so.dpb_pga_tangent_gram(3, 3, 4, 64, 10, 2, one, big, one, one, one, one, 1024, None) != 0 and "dpb_pga_scratch_bytes(3, 3, 4, 64, 2)" in msg()
    assert so.dpb_pga_tangent_gram(3, 3, 4, 64, 10, 2, one, 1024, one, one, one, one, big, None) != 0 and "dpb_frechet_scratch_bytes(3, 4, 64, 10)" in msg()
    assert so.dpb_pga_eig(None, 3, 3, 4, 64, 2, 1, 1, one, one, one, big, None) != 0 and "null" in msg()
    assert so.dpb_pga_eig(one, 3, 3, 4, 64, 2, 3, 1, one, one, one, big, None) != 0 and "M=3 outside" in msg()
    assert so.dpb_pga_eig(one, 3, 3, 4, 64, 2, 0, 1, one, one, one, big, None) != 0 and "M=0 outside" in msg()
    assert so.dpb_pga_eig(one, 3, 3, 4, 64, 2, 1, 1, one, one, one, 1024, None) != 0 and "dpb_pga_scratch_bytes" in msg()
    assert so.dpb_pga_combine(one, one, 1, None, 3, 3, 4, 64, 10, 2, one, big, one, big, None) != 0 and "null" in msg()
    assert so.dpb_pga_combine(one, one, 3, one, 3, 3, 4, 64, 10, 2, one, big, one, big, None) != 0 and "3 weight rows outside [1,J=2]" in msg()
    assert so.dpb_pga_combine(one, one, 1, one, 3, 3, 4, 64, 10, 2, one, big, one, 1024, None) != 0 and "dpb_pga_scratch_bytes" in msg()
    assert so.dpb_debug_set(b"pga_route", 0) == 0
    from diffusion_pullback_amd import geometry
    with pytest.raises(lib.DpbError, match="HIP device"):
        geometry.grassmann_pga(torch.zeros(2, 4, 64))
