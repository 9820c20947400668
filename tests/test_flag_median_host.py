"""CPU checks of the weighted flag mean and the flag median: tests/_flag_median_ref.py -- the float64 ambient-space reference the GPU tests measure
against -- is held to the unweighted reference, to the flag mean of a subset and to cases whose answer is closed-form, and to the conditions under which
the GPU tests make their claims; then the new entry points (exported, declared, arguments checked before any GPU call), the CLI flags and the cache
names of the median job."""
import os

import numpy as np
import pytest
import torch

import _flag_median_ref as M
import _flag_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_uniform_weights_give_the_unweighted_reference():
    a = R.graded_set(np.random.default_rng(0), 7, 5, 131)
    y0, i0 = R.flag_mean_ref(a, 3)
    for w in (None, np.ones(7), np.full(7, 2.5)):
        y, info = M.weighted_flag_mean_ref(a, 3, w)
        assert R.max_angle(y, y0) <= 1e-12 and np.abs(info["weight"] - i0["weight"]).max() <= 1e-13
        assert np.abs(info["theta"] - i0["theta"]).max() <= 1e-9 and np.abs(info["member_weight"] - 1).max() <= 1e-15


def test_zero_one_weights_give_the_flag_mean_of_the_subset():
    a = R.graded_set(np.random.default_rng(1), 9, 4, 80)
    mask = np.array([1, 0, 1, 1, 0, 1, 1, 1, 0], bool)
    y0, i0 = R.flag_mean_ref(a[mask], 3)
    y, info = M.weighted_flag_mean_ref(a, 3, mask.astype(float))
    assert R.max_angle(y, y0) <= 1e-12 and np.abs(info["weight"] - i0["weight"]).max() <= 1e-13
    assert info["theta"].shape == (9, 3) and np.abs(info["theta"][mask] - i0["theta"]).max() <= 1e-9
    assert np.abs(info["affinity"] - np.sum(np.cos(info["theta"]) ** 2, axis=1)).max() <= 1e-12


def test_one_member_is_its_own_median():
    eps = 1e-5
    a = R.clustered_set(np.random.default_rng(2), 1, 3, 40)
    y, info = M.flag_median_ref(a, 3, eps=eps)
    assert R.max_angle(y, a[0]) <= 1e-12 and info["converged"] and info["rounds"] == 1
    # d^2 = r - a is rounding noise of size r 2^-52: phi = eps / 2 + d^2 / (2 eps)
    assert np.abs(info["objective"] - eps / 2).max() <= 1e-4 * eps / 2
    assert np.isfinite(info["member_weight"]).all() and info["member_weight"][0] == 1.0


@pytest.mark.parametrize("theta", [0.3, 1.1])
def test_two_lines_hold_the_same_objective_along_their_geodesic(theta):
    """two members of rank 1 at angle theta: no single point is singled out along the geodesic between them (the sum of the two ANGLES is constant
    on it; the sum of sines, sin(t) + sin(theta - t), lies in [sin(theta), 2 sin(theta / 2)]), so only the objective is asserted: it starts at the
    bisector's 2 sin(theta / 2) -- the flag mean -- never rises, and cannot fall below sin(theta)"""
    e = np.eye(2, 12)
    a = np.stack([e[:1], np.cos(theta) * e[:1] + np.sin(theta) * e[1:2]])
    y, info = M.flag_median_ref(a, 1, max_rounds=500, tol=1e-14)
    assert info["monotone"]
    assert info["objective"][0] == pytest.approx(2 * np.sin(theta / 2), rel=1e-12)          # the flag mean: the bisector
    assert info["objective"][-1] >= np.sin(theta) * (1 - 1e-9) and info["objective"][-1] <= info["objective"][0]


def test_phi_is_the_huber_form():
    eps = 1e-3
    d = np.array([0.0, 0.5e-3, 1e-3, 2e-3, 1.0])
    assert np.allclose(M.phi(d, eps), [eps / 2, 0.125e-3 + 0.5e-3, 1e-3, 2e-3, 1.0], rtol=1e-15)


SMALL = [i for i, p in enumerate(M.PLANTED) if p[0][2] * (p[0][0] + p[0][1]) * p[0][3] <= 50000]      # (rows times length)


def test_planted_sets_meet_the_conditions():
    """the small planted sets here (the two large ones run with the GPU tests): they converge, descend, qualify; on the out_shared ones the median is
    at less than half the mean's angle from the planted frame and every inlier outweighs every outlier"""
    assert len(SMALL) == 4
    for idx in SMALL:
        (b_in, b_out, k, n, r), seed, shared = M.PLANTED[idx]
        a, frame = M.planted(np.random.default_rng(seed), b_in, b_out, k, n, r, out_shared=shared)
        assert a.dtype == np.float32 and a.shape == (b_in + b_out, k, n)
        y, info = M.flag_median_ref(a, r)
        assert info["converged"] and info["monotone"] and M.qualifies(info), M.PLANTED[idx]
        assert 1 <= info["rounds"] <= 50 and len(info["gaps"]) == len(info["dmin"]) == info["rounds"] + 1
        if shared:
            ym, _ = M.weighted_flag_mean_ref(a, r)
            assert R.max_angle(y, frame) < 0.5 * R.max_angle(ym, frame)
            assert info["member_weight"][:b_in].min() > info["member_weight"][b_in:].max()
        # a perturbation of 1e-12 relative moves the objective by far less than the GPU tests' bar of 1e-9
        rng = np.random.default_rng(9)
        _, i2 = M.flag_median_ref(a.astype(np.float64) * (1 + 1e-12 * rng.standard_normal(a.shape)), r)
        assert i2["rounds"] == info["rounds"] and (np.abs(i2["objective"] - info["objective"]) / info["objective"]).max() <= 1e-10


def test_prior_weights_enter_the_objective_and_the_reweighting():
    (b_in, b_out, k, n, r), seed, shared = M.PLANTED[0]
    a, _ = M.planted(np.random.default_rng(seed), b_in, b_out, k, n, r, out_shared=shared)
    p = np.ones(len(a))
    p[-3:] = 0.0
    y, info = M.flag_median_ref(a, r, weights=p)
    y2, i2 = M.flag_median_ref(a[:-3], r)
    assert R.max_angle(y, y2) <= 1e-9 and (info["member_weight"][-3:] == 0).all()
    assert np.abs(info["objective"] * (len(a) - 3) / len(a) - i2["objective"]).max() <= 1e-9


# ------------------------------------------------------------------------------------------------------------ the entry points
NAMES = ("dpb_flag_median_scratch_bytes", "dpb_flag_median_solver_bytes", "dpb_flag_median_init", "dpb_flag_median_iterate", "dpb_flag_median_round",
         "dpb_flag_median_finish")


def _lib():
    from diffusion_pullback_amd import lib
    return lib, lib.load()


def test_symbols_are_exported_and_declared():
    lib, so = _lib()
    header = open(os.path.join(ROOT, "include", "dpb.h")).read()
    for name in NAMES:
        assert name in lib.SYMBOLS and getattr(so, name) is not None and name in header, name
    assert so.dpb_abi_version() == 1


def test_scratch_bytes():
    _, so = _lib()
    f, g = so.dpb_flag_median_scratch_bytes, so.dpb_flag_median_solver_bytes
    up = lambda b: (b + 255) // 256 * 256
    B, k, r = 7, 5, 3
    own = up(64) + 4 * up(B * 8) + up(B * k * 8) + up(64 * 4) + up((72 + B) * 8)
    assert g(B, k, r, 100) == own + so.dpb_flag_mean_solver_bytes(B, k, r, 100)
    assert f(B, k, 131, r, 100) == own + so.dpb_flag_mean_scratch_bytes(B, k, 131, r, 100)
    assert f(100, 50, 196608, 10, 200) < so.dpb_flag_mean_scratch_bytes(100, 50, 196608, 10, 200) + (1 << 20)      # no second Gram
    for b, kk, n, rr, c in [(0, 4, 16, 1, 10), (65536, 4, 16, 1, 10), (2, 0, 16, 1, 10), (2, 65, 128, 1, 10), (2, 8, 7, 1, 10), (2, 4, 16, 0, 10),
                            (2, 4, 16, 9, 10), (40, 4, 128, 65, 10), (2, 4, 16, 1, -1)]:
        assert f(b, kk, n, rr, c) == 0, (b, kk, n, rr, c)
    assert f(2, 4, 16, 8, 10) > 0                                # a weighted mean takes r <= min(64, B k, N); the round refuses r > k
    assert g(2, 4, 9, 10) == 0 and g(2, 4, 8, 10) > 0


def test_arguments_are_checked_before_any_gpu_call():
    lib, so = _lib()
    msg = lambda: so.dpb_last_error().decode()
    one = 256                                                    # any aligned non-null value: the checks below fail before a pointer is used
    big = 1 << 30
    init, it, rnd, fin = so.dpb_flag_median_init, so.dpb_flag_median_iterate, so.dpb_flag_median_round, so.dpb_flag_median_finish
    assert init(None, None, None, 2, 4, 64, 2, 0, 10, one, big, None) != 0 and "exactly one of X and Ghat" in msg()
    assert init(one, one, None, 2, 4, 64, 2, 0, 10, one, big, None) != 0 and "exactly one of X and Ghat" in msg()
    assert init(one, None, None, 2, 4, 64, 2, 0, 10, None, big, None) != 0 and "null" in msg()
    assert init(one, None, None, 2, 4, 64, 9, 0, 10, one, big, None) != 0 and "r=9 outside" in msg()
    assert init(one, None, None, 2, 4, 64, 0, 0, 10, one, big, None) != 0 and "r=0 outside" in msg()
    assert init(one, None, None, 2, 65, 128, 2, 0, 10, one, big, None) != 0 and "k=65 outside [1,64]" in msg()
    assert init(one, None, None, 2, 4, 64, 2, 0, 10, one + 8, big, None) != 0 and "256-byte aligned" in msg()
    assert init(one, None, one, 2, 4, 64, 2, 0, 10, one, 1024, None) != 0 and "dpb_flag_median_scratch_bytes(2, 4, 64, 2, 10)" in msg()
    assert init(None, one, None, 2, 4, 64, 2, 0, 10, one, 1024, None) != 0 and "dpb_flag_median_solver_bytes(2, 4, 2, 10)" in msg()
    assert init(None, one + 8, None, 2, 4, 64, 2, 0, 10, one, big, None) != 0 and "32-byte aligned" in msg()
    assert it(-1, 1e-12, None, 2, 4, 64, 2, 10, one, big, None) != 0 and "n_iter" in msg()
    assert it(1, -1.0, None, 2, 4, 64, 2, 10, one, big, None) != 0 and "tol" in msg()
    assert it(1, 1e-12, None, 2, 4, 64, 2, 10, None, big, None) != 0 and "null" in msg()
    assert it(1, 1e-12, None, 2, 4, 64, 2, 10, one, 1024, None) != 0 and "dpb_flag_median_scratch_bytes" in msg()
    assert rnd(1e-5, 1e-9, 1, None, 2, 4, 64, 5, 10, one, big, None) != 0 and "r=5 outside [1,k=4]" in msg()
    assert rnd(0.0, 1e-9, 1, None, 2, 4, 64, 2, 10, one, big, None) != 0 and "eps=0" in msg()
    assert rnd(1e-5, -1.0, 1, None, 2, 4, 64, 2, 10, one, big, None) != 0 and "tol" in msg()
    assert rnd(1e-5, 1e-9, 1, None, 2, 4, 64, 2, 10, None, big, None) != 0 and "null" in msg()
    assert rnd(1e-5, 1e-9, 1, None, 2, 4, 64, 2, 10, one, 1024, None) != 0 and "dpb_flag_median_scratch_bytes" in msg()
    assert fin(one, None, one, one, one, one, None, one, 2, 4, 64, 2, 10, one, big, None) != 0 and "null" in msg()
    assert fin(one, None, None, one, one, one, one, one, 2, 4, 64, 2, 10, one, big, None) != 0 and "X and Y go together" in msg()
    assert fin(one, None, one, one, one, one, one, one, 2, 4, 64, 2, 10, one, 1024, None) != 0 and "dpb_flag_median_scratch_bytes" in msg()
    from diffusion_pullback_amd import geometry
    with pytest.raises(lib.DpbError, match="HIP device"):
        geometry.flag_median(torch.zeros(2, 4, 64))
    with pytest.raises(lib.DpbError, match="HIP device"):
        geometry.flag_mean(torch.zeros(2, 4, 64), weights=[1.0, 1.0])


# ------------------------------------------------------------------------------------------------------------ the job and the CLI
def test_cli_flags_parse(capsys):
    from diffusion_pullback_amd import main as m
    a = m.parse_args(["--note", "t"])
    assert (a.flag_mean_kind, a.flag_median_eps, a.flag_median_max_rounds) == ("mean", 1e-5, 50)
    a = m.parse_args(["--note", "t", "--run_edit_global_flag_mean_zt", "True", "--flag_mean_kind", "median", "--flag_median_eps", "1e-4",
                      "--flag_median_max_rounds", "7", "--model_name", "CelebA_HQ_HF", "--pca_rank", "50", "--flag_rank", "10"])
    assert (a.flag_mean_kind, a.flag_median_eps, a.flag_median_max_rounds, a.flag_rank) == ("median", 1e-4, 7, 10)
    capsys.readouterr()
    for model_flags in (["--run_edit_global_flag_mean_zt", "True", "--flag_mean_kind", "median"], ["--flag_mean_kind", "median"]):
        with pytest.raises(SystemExit):
            m.parse_args(["--note", "t", "--model_name", "runwayml/stable-diffusion-v1-5"] + model_flags)
        assert "Stable Diffusion" in capsys.readouterr().err
    for bad in (["--flag_mean_kind", "mode"], ["--flag_median_eps", "0"], ["--flag_median_eps", "-1e-5"], ["--flag_median_max_rounds", "-1"]):
        with pytest.raises(SystemExit):
            m.parse_args(["--note", "t", "--run_edit_global_flag_mean_zt", "True"] + bad)
    capsys.readouterr()
    for flag in ("--flag_mean_kind", "--flag_median_eps", "--flag_median_max_rounds"):
        assert flag in m.__doc__


def _driver(tmp):
    from diffusion_pullback_amd import main as m
    from diffusion_pullback_amd.edit import EditUncondDiffusion
    argv = ["--note", "t", "--model_name", "CelebA_HQ_HF", "--dataset_name", "CelebA_HQ", "--result_folder", str(tmp), "--device", "cpu",
            "--performance_boosting_t", "0.2", "--h_t", "0.8", "--edit_t", "0.6", "--seed", "0"]
    args = m.preset(m.parse_args(argv))
    args.for_steps = args.inv_steps = 20
    args.input_root = os.path.join(str(tmp), "inputs")
    return args, EditUncondDiffusion(args, unet=None)


def test_cache_names_and_argument_errors(tmp_path):
    args, ed = _driver(tmp_path)
    for space, tag in (("x", "v"), ("h", "u")):
        today = ed.global_flag_mean_paths("mid", 0, 4, 8, space, flag_rank=2)
        assert ed.global_flag_mean_paths("mid", 0, 4, 8, space, flag_rank=2, flag_mean_kind="mean") == today
        assert os.path.basename(today[0]) == f"{tag}-0.8T-mid-block_0-seed_0-num_local_basis_8-rank_2.pt"
        basis, info = ed.global_flag_mean_paths("mid", 0, 4, 8, space, flag_rank=2, flag_mean_kind="median")
        assert os.path.dirname(basis) == os.path.dirname(today[0]) == os.path.dirname(info)
        assert os.path.basename(basis) == f"{tag}-0.8T-mid-block_0-seed_0-num_local_basis_8-rank_2-median.pt"
        assert os.path.basename(info) == "info-" + os.path.basename(basis)
    with pytest.raises(ValueError, match="flag_mean_kind must be"):
        ed.global_flag_mean_paths("mid", 0, 4, 8, "x", flag_mean_kind="mode")
    with pytest.raises(ValueError, match="flag_mean_kind must be"):
        ed.run_edit_global_flag_mean_zt(0, vis_num=4, vis_num_pc=1, pca_rank=4, num_local_basis=4, flag_mean_kind="mode")
    with pytest.raises(ValueError, match="flag_rank = 5 outside"):
        ed.run_edit_global_flag_mean_zt(0, vis_num=4, vis_num_pc=1, pca_rank=4, num_local_basis=4, flag_rank=5, flag_mean_kind="median")
    assert os.listdir(args.result_folder) == [] and not os.path.exists(args.input_root)
