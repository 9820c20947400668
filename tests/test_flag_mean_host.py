"""CPU checks of the flag (extrinsic) mean: tests/_flag_ref.py -- the float64 ambient-space reference the GPU tests measure against -- is held to
constructions whose answer is closed-form; the numpy restatement of the kernel's method (block subspace iteration on the whitened Gram) is held to the
reference at the GPU tests' bars; then the new entry points (exported, declared, arguments checked before any GPU call), the CLI flags and the cache
names of run_edit_global_flag_mean_zt."""
import os

import numpy as np
import pytest
import torch

import _flag_ref as R
import _grassmann_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-6
EPS = 4 * 2.0 ** -24


def test_identical_members_give_their_span_with_weight_one():
    rng = np.random.default_rng(0)
    q = rng.standard_normal((4, 50))
    a = np.stack([R.mixing(rng, 4, 30.0) @ q for _ in range(5)])
    y, info = R.flag_mean_ref(a)
    assert R.max_angle(y, q) <= 1e-12 and np.abs(info["weight"] - 1).max() <= 1e-12
    assert np.abs(info["eigenvalues"][4:]).max() <= 1e-12 and np.abs(info["theta"]).max() <= BAR


def test_one_shared_vector_on_disjoint_blocks():
    """B members on disjoint coordinate blocks plus one exactly shared vector: weight 1 for it, 1 / B for every other direction"""
    b, k, blk = 4, 3, 7
    n = 1 + b * blk
    rng = np.random.default_rng(1)
    a = np.zeros((b, k, n))
    for i in range(b):
        a[i, 0, 0] = 1.0
        a[i, 1:, 1 + i * blk:1 + (i + 1) * blk] = rng.standard_normal((k - 1, blk))
        a[i] = R.mixing(rng, k, 10.0) @ a[i]
    y, info = R.flag_mean_ref(a, 3)
    assert abs(abs(y[0, 0]) - 1) <= 1e-12 and abs(info["weight"][0] - 1) <= 1e-12
    assert np.abs(info["eigenvalues"][1:b * (k - 1) + 1] - 1 / b).max() <= 1e-12
    assert R.rel_gaps(info["eigenvalues"])[0] == pytest.approx(1 - 1 / b)


def test_two_members_give_the_geodesic_midpoint():
    rng = np.random.default_rng(2)
    a, b_ = G.planted_pair(rng, 4, 40, np.array([1.2, 0.7, 0.3, 0.05]))
    y, info = R.flag_mean_ref(np.stack([a, b_]))
    mid = G.geodesic(a, b_, [0.5])[0]
    th = R.angles_to(a, b_)
    assert R.max_angle(y, mid) <= 1e-12
    assert np.abs(info["weight"] - np.sort((1 + np.cos(th)) / 2)[::-1]).max() <= 1e-12


@pytest.mark.parametrize("kind,b,k,n,r", [("graded", 7, 5, 131, 3), (0.6, 7, 5, 131, 5), ("graded", 33, 2, 40, 1), ("graded", 5, 16, 517, 4), (0.5, 2, 3, 64, 3)])
def test_the_methods_restatement_meets_the_gpu_bars(kind, b, k, n, r):
    rng = np.random.default_rng(100 * b + k + r)
    noise = {1: (0.1,), 3: (0.1, 0.45, 0.87), 4: (0.1, 0.3, 0.6, 0.9)}
    a = R.graded_set(rng, b, k, n, noise[r]) if kind == "graded" else R.clustered_set(rng, b, k, n, spread=kind)
    yr, ir = R.flag_mean_ref(a, r)
    ym, im = R.flag_mean_method(a, r)
    gaps = R.rel_gaps(ir["eigenvalues"])
    assert gaps[r - 1] >= 0.05
    angs = [R.max_angle(ym[:j], yr[:j]) for j in range(1, r + 1) if gaps[j - 1] >= 0.05]
    print(f"{kind} B={b} k={k} N={n} r={r}: {im['iterations']} iterations, residual {im['residual']:.1e}, angles {max(angs):.1e}, weight "
          f"{np.abs(im['weight'] - ir['weight']).max():.1e}")
    assert im["converged"] and im["iterations"] <= 60
    assert max(angs) <= BAR and np.abs(im["weight"] - ir["weight"]).max() <= EPS and np.abs(ym @ ym.T - np.eye(r)).max() <= EPS
    assert np.abs(R.rayleigh_weights(a, ym) - im["weight"]).max() <= 1e-12
    assert len(im["eigenvalues"]) == R.block_width(b * k, r)


def test_the_restatement_returns_rayleigh_quotients_when_it_has_not_converged():
    a = R.spread_set(np.random.default_rng(6), b=6, k=6, n=2048)
    ym, im = R.flag_mean_method(a, 3, max_iter=8)
    assert not im["converged"] and im["iterations"] == 8
    assert np.abs(ym @ ym.T - np.eye(3)).max() <= 1e-12 and np.abs(R.rayleigh_weights(a, ym) - im["weight"]).max() <= 1e-12


def test_the_restatement_survives_a_rank_deficient_gram():
    """identical members: Ghat has rank k and the block is wider -- the dropped directions leave the kept ones orthonormal"""
    rng = np.random.default_rng(3)
    q = rng.standard_normal((3, 30))
    a = np.stack([R.mixing(rng, 3, 5.0) @ q for _ in range(9)])
    ym, im = R.flag_mean_method(a, 3)
    assert im["converged"] and R.max_angle(ym, q) <= 1e-9 and np.abs(im["weight"] - 1).max() <= 1e-12
    assert np.abs(im["eigenvalues"][3:]).max() <= 1e-9


# ------------------------------------------------------------------------------------------------------------ the entry points
NAMES = ("dpb_flag_mean_scratch_bytes", "dpb_flag_mean_solver_bytes", "dpb_flag_mean_init", "dpb_flag_mean_iterate", "dpb_flag_mean_finish",
         "dpb_frechet_start", "dpb_frechet_ghat")


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
    f, g = so.dpb_flag_mean_scratch_bytes, so.dpb_flag_mean_solver_bytes
    up = lambda b: (b + 255) // 256 * 256
    B, k, r = 7, 5, 3
    R_, m = B * k, 16
    solver = up(32) + 3 * up(R_ * m * 8) + up(1 * 2 * m * m * 8) + up(1 * m * 8) + up(2 * m * m * 8 + 2 * 64 * 8)
    assert g(B, k, r, 100) == solver
    assert f(B, k, 131, r, 100) == solver + up(B * k * k * 8) + up(B * 4) + up(R_ * R_ * 8)
    assert f(100, 50, 196608, 50, 1000) > 8 * 5000 * 5000 and f(1, 1, 5, 1, 0) > 0 and f(33, 2, 40, 1, 10) > 0
    for b, kk, n, rr, c in [(0, 4, 16, 1, 10), (65536, 4, 16, 1, 10), (2, 0, 16, 1, 10), (2, 65, 128, 1, 10), (2, 8, 7, 1, 10), (2, 4, 16, 0, 10),
                            (2, 4, 16, 9, 10), (20, 4, 16, 17, 10), (40, 4, 128, 65, 10), (2, 4, 16, 1, -1)]:
        assert f(b, kk, n, rr, c) == 0, (b, kk, n, rr, c)
    assert g(2, 4, 9, 10) == 0 and g(2, 4, 8, 10) > 0


def test_arguments_are_checked_before_any_gpu_call():
    lib, so = _lib()
    msg = lambda: so.dpb_last_error().decode()
    one = 256                                                    # any aligned non-null value: the checks below fail before a pointer is used
    big = 1 << 30
    assert so.dpb_flag_mean_init(None, None, 2, 4, 64, 2, 0, 10, one, big, None) != 0 and "exactly one of X and Ghat" in msg()
    assert so.dpb_flag_mean_init(one, one, 2, 4, 64, 2, 0, 10, one, big, None) != 0 and "exactly one of X and Ghat" in msg()
    assert so.dpb_flag_mean_init(one, None, 2, 4, 64, 2, 0, 10, None, big, None) != 0 and "null" in msg()
    assert so.dpb_flag_mean_init(one, None, 2, 4, 64, 9, 0, 10, one, big, None) != 0 and "r=9 outside" in msg()
    assert so.dpb_flag_mean_init(one, None, 2, 4, 64, 0, 0, 10, one, big, None) != 0 and "r=0 outside" in msg()
    assert so.dpb_flag_mean_init(one, None, 2, 65, 128, 2, 0, 10, one, big, None) != 0 and "k=65 outside [1,64]" in msg()
    assert so.dpb_flag_mean_init(one, None, 2, 4, 64, 2, 0, 10, one + 8, big, None) != 0 and "256-byte aligned" in msg()
    assert so.dpb_flag_mean_init(one, None, 2, 4, 64, 2, 0, 10, one, 1024, None) != 0 and "dpb_flag_mean_scratch_bytes(2, 4, 64, 2, 10)" in msg()
    assert so.dpb_flag_mean_init(None, one, 2, 4, 64, 2, 0, 10, one, 1024, None) != 0 and "dpb_flag_mean_solver_bytes(2, 4, 2, 10)" in msg()
    assert so.dpb_flag_mean_init(None, one + 8, 2, 4, 64, 2, 0, 10, one, big, None) != 0 and "32-byte aligned" in msg()
    assert so.dpb_flag_mean_iterate(-1, 1e-12, None, 2, 4, 64, 2, 10, one, big, None) != 0 and "n_iter" in msg()
    assert so.dpb_flag_mean_iterate(1, -1.0, None, 2, 4, 64, 2, 10, one, big, None) != 0 and "tol" in msg()
    assert so.dpb_flag_mean_iterate(1, 1e-12, None, 2, 4, 64, 2, 10, None, big, None) != 0 and "null" in msg()
    assert so.dpb_flag_mean_finish(one, None, one, one, one, one, None, 2, 4, 64, 2, 10, one, big, None) != 0 and "null" in msg()
    assert so.dpb_flag_mean_finish(one, None, None, one, one, one, one, 2, 4, 64, 2, 10, one, big, None) != 0 and "X and Y go together" in msg()
    assert so.dpb_flag_mean_finish(one, None, one, one, one, one, one, 2, 4, 64, 2, 10, one, 1024, None) != 0 and "dpb_flag_mean_scratch_bytes" in msg()
    assert so.dpb_frechet_start(None, 2, 4, 64, 10, one, big, None) != 0 and "null" in msg()
    assert so.dpb_frechet_start(one, 2, 4, 64, 10, one + 8, big, None) != 0 and "256-byte aligned" in msg()
    assert so.dpb_frechet_start(one, 2, 4, 64, 10, one, 1024, None) != 0 and "dpb_frechet_scratch_bytes(2, 4, 64, 10)" in msg()
    assert so.dpb_frechet_ghat(2, 65, 128, 10, one) is None and "no Frechet problem" in msg()
    assert so.dpb_frechet_ghat(2, 4, 64, 10, 1 << 20) == (1 << 20) + 256         # Ghat follows the status block
    from diffusion_pullback_amd import geometry
    with pytest.raises(lib.DpbError, match="HIP device"):
        geometry.flag_mean(torch.zeros(2, 4, 64))


# ------------------------------------------------------------------------------------------------------------ the job and the CLI
def test_cli_flags_parse(capsys):
    from diffusion_pullback_amd import main as m
    a = m.parse_args(["--note", "t"])
    assert a.run_edit_global_flag_mean_zt is False and (a.flag_mean_space, a.flag_rank, a.frechet_init) == ("x", 0, "member")
    a = m.parse_args(["--note", "t", "--run_edit_global_flag_mean_zt", "True", "--flag_mean_space", "h", "--flag_rank", "10", "--num_local_basis", "100",
                      "--model_name", "CelebA_HQ_HF", "--pca_rank", "50"])
    assert a.run_edit_global_flag_mean_zt is True and (a.flag_mean_space, a.flag_rank, a.num_local_basis) == ("h", 10, 100)
    a = m.parse_args(["--note", "t", "--run_edit_global_frechet_mean_zt", "True", "--frechet_init", "flag"])
    assert a.frechet_init == "flag"
    capsys.readouterr()
    with pytest.raises(SystemExit):
        m.parse_args(["--note", "t", "--run_edit_global_flag_mean_zt", "True", "--model_name", "runwayml/stable-diffusion-v1-5"])
    err = capsys.readouterr().err
    assert "Stable Diffusion" in err and "unconditional" in err
    for bad in (["--flag_mean_space", "z"], ["--flag_mean_space", "h", "--local_projection", "False"], ["--flag_rank", "3"], ["--flag_rank", "-1"]):
        with pytest.raises(SystemExit):
            m.parse_args(["--note", "t", "--run_edit_global_flag_mean_zt", "True"] + bad)          # (pca_rank defaults to 2)
    with pytest.raises(SystemExit):
        m.parse_args(["--note", "t", "--frechet_init", "mean"])
    capsys.readouterr()
    for flag in ("--run_edit_global_flag_mean_zt", "--flag_mean_space", "--flag_rank", "--frechet_init"):
        assert flag in m.__doc__


def test_engine_sizing_covers_the_local_bases(tmp_path):
    from diffusion_pullback_amd import main as m
    argv = ["--note", "t", "--model_name", "CelebA_HQ_HF", "--dataset_name", "Random", "--result_folder", str(tmp_path), "--device", "cpu",
            "--performance_boosting_t", "0.2", "--run_edit_global_flag_mean_zt", "True", "--num_local_basis", "8", "--pca_rank", "3"]
    a = m.preset(m.parse_args(argv))
    assert m.frechet_group(a) == 8


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
        for rank, r in ((None, 4), (0, 4), (2, 2)):
            basis, info = ed.global_flag_mean_paths("mid", 0, 4, 8, space, flag_rank=rank)
            assert os.path.basename(os.path.dirname(basis)) == "global_flag_mean_uncond-model_CelebA_HQ_HF-dataset_CelebA_HQ-num_steps_20-pca_rank_4"
            assert os.path.basename(basis) == f"{tag}-0.8T-mid-block_0-seed_0-num_local_basis_8-rank_{r}.pt"
            assert os.path.basename(info) == "info-" + os.path.basename(basis) and os.path.dirname(info) == os.path.dirname(basis)
    run = lambda **kw: ed.run_edit_global_flag_mean_zt(0, vis_num=4, pca_rank=4, num_local_basis=4, **kw)
    with pytest.raises(ValueError, match="flag_mean_space must be"):
        run(vis_num_pc=1, flag_mean_space="z")
    with pytest.raises(ValueError, match="local_projection=False is valid for flag_mean_space 'x' only"):
        run(vis_num_pc=1, flag_mean_space="h", local_projection=False)
    with pytest.raises(ValueError, match="flag_rank = 5 outside"):
        run(vis_num_pc=1, flag_rank=5)
    with pytest.raises(ValueError, match=r"2 rows: pcs \[0, 1, 2\]"):
        run(vis_num_pc=3, flag_rank=2)
    with pytest.raises(ValueError, match="2 rows"):
        run(vis_pc_list=[2], flag_rank=2)
    with pytest.raises(ValueError, match="frechet_init must be"):
        ed.run_edit_global_frechet_mean_zt(0, vis_num=4, vis_num_pc=1, pca_rank=4, num_local_basis=4, frechet_init="mean")
    assert os.listdir(args.result_folder) == [] and not os.path.exists(args.input_root)
