"""Host checks of the least-squares inverse (no GPU): the float64 restatement of tests/_cgls_ref.py against the dense solve, scipy's LSQR and the
identity of the first iterate; the frozen-row hand-through; the refusals of the C entry points (they come before any launch); the parser rules of
--edit_xt newton-h."""
import ctypes as C

import numpy as np
import pytest

import _cgls_ref as R


def _problem(seed, D=14, N=9, rank=None, rows=3):
    g = np.random.default_rng(seed)
    Js, cs = [], []
    for _ in range(rows):
        J = g.standard_normal((D, N))
        if rank is not None:
            J = g.standard_normal((D, rank)) @ g.standard_normal((rank, N))
        Js.append(J); cs.append(g.standard_normal(D))
    return Js, np.stack(cs)


def _solve(Js, c, **kw):
    matvec = lambda p: np.stack([J @ v for J, v in zip(Js, p)])
    rmatvec = lambda r: np.stack([J.T @ v for J, v in zip(Js, r)])
    return R.solve_ref(matvec, rmatvec, c, store=np.float64, **kw)


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("mu", [0.0, 0.3, 5.0])
def test_the_restatement_reaches_the_dense_solution(mu):
    Js, c = _problem(1)
    S, hist = _solve(Js, c, mu_abs=mu, tol=1e-13, iters=30)
    for b, J in enumerate(Js):
        assert _rel(S.delta[b], R.dense_solve(J, c[b], mu)) <= 1e-10, (mu, b)
    assert (hist[-1, :, 3] == 1).all() and (S.state[:, R.ITERS] <= 12).all()           # N = 9 directions: converged, then frozen
    assert np.allclose(hist[-1, :, 1], [np.linalg.norm(c[b] - J @ S.delta[b]) ** 2 for b, J in enumerate(Js)], rtol=1e-9)
    assert np.allclose(hist[-1, :, 2], (S.delta ** 2).sum(axis=1), rtol=1e-12)


def test_mu_rel_is_in_units_of_the_squared_gain_along_c():
    Js, c = _problem(2)
    S, _ = _solve(Js, c, mu_abs=0.01, mu_rel=0.2, tol=1e-13, iters=30)
    for b, J in enumerate(Js):
        mu_b = 0.01 + 0.2 * np.linalg.norm(J.T @ c[b]) ** 2 / np.linalg.norm(c[b]) ** 2
        assert abs(S.state[b, R.MU] - mu_b) <= 1e-14 * mu_b
        assert _rel(S.delta[b], R.dense_solve(J, c[b], mu_b)) <= 1e-10
    # a pure left singular direction: the step shrinks by 1 / (1 + mu_rel)
    U, s, Vt = np.linalg.svd(Js[0], full_matrices=False)
    S, _ = _solve(Js[:1], U[:, 2][None], mu_rel=0.25, tol=1e-13, iters=5)
    assert _rel(S.delta[0], Vt[2] / s[2] / 1.25) <= 1e-12


@pytest.mark.parametrize("rank", [3, 6])
def test_rank_deficient_at_mu_zero_gives_the_minimum_norm_solution(rank):
    Js, c = _problem(3, rank=rank)
    S, hist = _solve(Js, c, tol=1e-12, iters=30)
    for b, J in enumerate(Js):
        assert _rel(S.delta[b], np.linalg.pinv(J) @ c[b]) <= 1e-9, (rank, b)
    assert (S.state[:, R.ITERS] <= rank + 2).all() and (hist[-1, :, 3] == 1).all()


@pytest.mark.parametrize("mu", [0.0, 0.3, 5.0])
def test_against_scipy_lsqr(mu):
    from scipy.sparse.linalg import lsqr
    Js, c = _problem(4)
    S, _ = _solve(Js, c, mu_abs=mu, tol=1e-14, iters=40)
    for b, J in enumerate(Js):
        x = lsqr(J, c[b], damp=np.sqrt(mu), atol=1e-15, btol=1e-15, conlim=0, iter_lim=200)[0]
        assert _rel(S.delta[b], x) <= 1e-10, (mu, b)


def test_the_first_iterate_is_parallel_to_the_gradient():
    Js, c = _problem(5)
    S, hist = _solve(Js, c, mu_abs=0.7, iters=1)
    for b, J in enumerate(Js):
        g = J.T @ c[b]
        cos = S.delta[b] @ g / (np.linalg.norm(S.delta[b]) * np.linalg.norm(g))
        assert cos >= 1 - 1e-12
        assert abs(hist[0, b, 0] - g @ g) <= 1e-12 * (g @ g) and abs(hist[0, b, 1] - c[b] @ c[b]) <= 1e-12 * (c[b] @ c[b]) and hist[0, b, 2] == 0


def test_a_frozen_row_is_handed_through():
    """tol = 0.5 freezes the rows at different rounds; from then on a row's vectors and scalars do not move, whatever comes in"""
    Js, c = _problem(6)
    matvec = lambda p: np.stack([J @ v for J, v in zip(Js, p)])
    rmatvec = lambda r: np.stack([J.T @ v for J, v in zip(Js, r)])
    S, _ = R.init_ref(c, rmatvec(c), 0.1, 0.0, 0.5, np.float64)
    frozen_at = {}
    for i in range(8):
        before = S.copy()
        q = matvec(S.p); q[list(frozen_at)] = np.nan
        R.h_step_ref(S, q)
        w = rmatvec(np.nan_to_num(S.r)); w[list(frozen_at)] = np.inf
        R.x_step_ref(S, w, 0.5)
        for b in frozen_at:
            assert all(np.array_equal(getattr(S, k)[b], getattr(before, k)[b]) for k in ("delta", "r", "p", "state")), (i, b)
        for b in range(3):
            if S.state[b, R.FLAG] == 1 and b not in frozen_at:
                frozen_at[b] = i
    assert len(frozen_at) == 3 and np.isfinite(S.delta).all()
    # gamma0 = 0 (c orthogonal to the range of J): frozen by init with flag 1, delta = 0
    S, h = R.init_ref(c, np.zeros((3, 9)), 0.1, 0.1, 0.0, np.float64)
    assert (h[:, 3] == 1).all() and (S.delta == 0).all()


def test_the_c_entry_points_refuse_by_name():
    from diffusion_pullback_amd import lib as L
    lib = L.load()
    assert lib.dpb_cgls_init_scratch_bytes(3, 4099, 4097) == 3 * (2 + 2) * 2 * 8
    assert lib.dpb_cgls_h_step_scratch_bytes(3, 4099, 4097) == lib.dpb_cgls_x_step_scratch_bytes(3, 4099, 4097) == 192
    assert lib.dpb_cgls_init_scratch_bytes(0, 5, 7) == 0 and lib.dpb_cgls_init_scratch_bytes(1, 0, 7) == 0 and lib.dpb_cgls_init_scratch_bytes(1, 5, 0) == 0
    P = 4096                                                   # never dereferenced: every refusal below comes before a launch

    def init(c=P, w0=P, R_=2, N=5, D=7, mu_abs=0.0, mu_rel=0.1, tol=1e-5, scratch=P, nbytes=1024, state=P, hist=P):
        return lib.dpb_cgls_init(c, w0, P, P, P, state, hist, mu_abs, mu_rel, tol, R_, N, D, scratch, nbytes, None)

    def refused(rc, word):
        assert rc != 0 and word.encode() in lib.dpb_last_error(), (word, lib.dpb_last_error())

    refused(init(c=None), "dpb_cgls_init: null argument")
    refused(init(scratch=None), "null argument")
    refused(init(R_=0), "R=0")
    refused(init(N=0), "N=0")
    refused(init(D=-1), "D=-1")
    refused(init(mu_abs=-1.0), "mu_abs")
    refused(init(mu_rel=float("nan")), "mu_rel")
    refused(init(tol=float("inf")), "tol")
    refused(init(nbytes=63), "scratch of 63 bytes")
    refused(init(scratch=P + 4), "8-byte aligned")
    refused(init(state=P + 4), "8-byte aligned")
    refused(lib.dpb_cgls_h_step(None, P, P, P, P, P, 2, 5, 7, P, 1024, None), "dpb_cgls_h_step: null argument")
    refused(lib.dpb_cgls_h_step(P, P, P, P, P, P, 2, 5, 0, P, 1024, None), "D=0")
    refused(lib.dpb_cgls_h_step(P, P, P, P, P, P, 2, 5, 7, P, 8, None), "scratch of 8 bytes")
    refused(lib.dpb_cgls_x_step(P, P, P, P, P, None, 0.0, 2, 5, 7, P, 1024, None), "dpb_cgls_x_step: null argument")
    refused(lib.dpb_cgls_x_step(P, P, P, P, P, P, -1e-3, 2, 5, 7, P, 1024, None), "tol")
    refused(lib.dpb_cgls_x_step(P, P, P, P, P, P, 0.0, 0, 5, 7, P, 1024, None), "R=0")
    one = (C.c_float * 1)(1.0)
    refused(lib.dpb_newton_residual(P, P, P, 2, (C.c_int32 * 1)(2), one, one, 0.5, 1, 7, P, None), "dir[0]=2")
    refused(lib.dpb_newton_residual(P, P, P, 2, (C.c_int32 * 1)(0), one, (C.c_float * 1)(float("nan")), 0.5, 1, 7, P, None), "scale[0]")
    refused(lib.dpb_newton_residual(P, None, P, 2, (C.c_int32 * 1)(0), one, one, 0.5, 1, 7, P, None), "null argument")
    refused(lib.dpb_newton_update(P, P, P, -1.0, P, P, 1, 5, None), "radius")
    refused(lib.dpb_newton_update(P, P, None, 0.0, P, P, 1, 5, None), "null argument")
    refused(lib.dpb_jac_lstsq(None, 0, P, 1, 0.0, 0.1, 1e-5, 4, P, None, P, P, 1024), "dpb_jac_lstsq: null argument")
    refused(lib.dpb_newton_h_chain(None, 0, P, 1, one, None, P, 1, (C.c_int32 * 1)(0), one, one, 2, 2, 0.0, 0.1, 1e-5, 0.0, 1, P, P, P, P, P, 1024),
            "dpb_newton_h_chain: null argument")
    assert lib.dpb_jac_lstsq_scratch_bytes(None, 0, 1) == 0 and lib.dpb_newton_h_chain_scratch_bytes(None, 0, 1) == 0


BASE = ["--note", "t", "--model_name", "CelebA_HQ_HF", "--dataset_name", "Random"]
JOB = ["--run_edit_global_frechet_mean_zt", "True", "--frechet_mean_space", "h"]


def _parse(extra):
    from diffusion_pullback_amd import main as m
    return m.parse_args(BASE + extra)


def test_the_parser_takes_newton_h_and_its_flags():
    a = _parse(JOB + ["--edit_xt", "newton-h", "--h_edit_step_size", "2.5", "--local_projection", "False"])
    assert a.edit_xt == "newton-h" and (a.newton_iters, a.newton_damping, a.newton_radius) == (8, 0.1, 0.0)
    a = _parse(JOB + ["--edit_xt", "newton-h", "--h_edit_step_size", "-1", "--newton_iters", "3", "--newton_damping", "0.5", "--newton_radius", "4"])
    assert (a.newton_iters, a.newton_damping, a.newton_radius) == (3, 0.5, 4.0)


@pytest.mark.parametrize("extra,word", [
    (JOB + ["--edit_xt", "newton-h"], "h_edit_step_size"),
    (["--run_edit_global_frechet_mean_zt", "True", "--frechet_mean_space", "x", "--edit_xt", "newton-h", "--h_edit_step_size", "1"], "frechet_mean_space must be h"),
    (["--run_edit_global_flag_mean_zt", "True", "--edit_xt", "newton-h", "--h_edit_step_size", "1"], "flag_mean_space must be h"),
    (["--run_edit_global_hungarian_mean_zt", "True", "--edit_xt", "newton-h", "--h_edit_step_size", "1"], "hungarian_mean_space must be h"),
    (JOB + ["--edit_xt", "newton-h", "--h_edit_step_size", "1", "--edit_ht", "h_space_guidance"], "exclude each other"),
    (JOB + ["--edit_xt", "newton-h", "--h_edit_step_size", "1", "--newton_iters", "-1"], "newton_iters"),
    (JOB + ["--edit_xt", "newton-h", "--h_edit_step_size", "1", "--newton_damping", "-0.1"], "newton_damping"),
    (JOB + ["--edit_xt", "sideways"], "newton-h"),
])
def test_the_parser_refuses(extra, word, capsys):
    with pytest.raises(SystemExit):
        _parse(extra)
    assert word in capsys.readouterr().err


def test_stable_diffusion_is_refused(capsys):
    from diffusion_pullback_amd import main as m
    with pytest.raises(SystemExit):
        m.parse_args(["--note", "t", "--model_name", "stable-diffusion-v1-5", "--edit_xt", "newton-h", "--h_edit_step_size", "1"])
    assert "newton-h" in capsys.readouterr().err


def test_the_default_namespace_is_unchanged_but_for_the_new_flags():
    a = vars(_parse([]))
    new = {"newton_iters": 8, "newton_damping": 0.1, "newton_radius": 0.0}
    assert {k: a[k] for k in new} == new
    assert a["edit_xt"] == "parallel-x" and a["edit_ht"] == "default" and a["h_edit_step_size"] == 0
    from diffusion_pullback_amd import main as m
    names = [f[0] for f in m._FLAGS]
    assert len(names) == len(set(names)) and all(k in names for k in new)
    # parallel-x and parallel-h parse exactly as before
    assert _parse(JOB + ["--edit_xt", "parallel-h", "--x_edit_step_size", "2"]).edit_xt == "parallel-h"


def test_the_driver_refuses_before_anything_is_computed():
    """_check_parallel_h, the first thing the three jobs do: space x, a zero shift, the guidance branch, a bad flag"""
    from diffusion_pullback_amd import edit as E

    class Stub:
        edit_xt, edit_ht, h_edit_step_size, x_edit_step_size = "newton-h", "default", 1.0, 0.0
        newton_iters, newton_damping, newton_radius = 8, 0.1, 0.0
        _check_h_guidance = E.EditUncondDiffusion._check_h_guidance

    check = E.EditUncondDiffusion._check_parallel_h
    check(Stub(), "h")
    with pytest.raises(ValueError, match="space 'h'"):
        check(Stub(), "x")
    for attr, val, word in (("h_edit_step_size", 0.0, "h_edit_step_size"), ("h_edit_step_size", float("nan"), "h_edit_step_size"),
                            ("newton_iters", -1, "newton_iters"), ("newton_radius", -1.0, "newton_radius"), ("edit_xt", "newton", "newton-h")):
        s = Stub(); setattr(s, attr, val)
        with pytest.raises(ValueError, match=word):
            check(s, "h")
    s = Stub(); s.edit_ht = "h_space_guidance"
    with pytest.raises(ValueError, match="exclude each other"):
        check(s, "h")
