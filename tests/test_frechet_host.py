"""CPU checks of the Grassmann Frechet mean: tests/_frechet_ref.py -- the float64 ambient-space restatement the GPU tests measure against -- is held to
constructions whose mean is known, all at 1e-6 rad, the project's bar for angles; then the names, skip rule and argument errors of
run_edit_global_frechet_mean_zt, its CLI flags, and the argument checks of the new entry points, which run before any GPU call."""
import os

import numpy as np
import pytest
import torch
from scipy.linalg import subspace_angles

import _frechet_ref as R
from _util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-6


def test_one_basis_is_its_own_mean_in_zero_steps():
    a = R.clustered_set(np.random.default_rng(0), 1, 5, 300)
    y, info = R.frechet_mean_ref(a)
    assert info["iterations"] == 0 and info["converged"] and info["cost"].tolist() == [info["cost"][0]] and info["cost"][0] <= 1e-20
    assert R.max_angle(y, a[0]) <= BAR and np.abs(y @ y.T - np.eye(5)).max() <= 1e-12
    assert np.abs(info["weight"] - 1).max() <= 1e-12


def test_two_bases_give_the_geodesic_midpoint():
    a = R.pair_set(np.random.default_rng(2), 6, 400)
    y, info = R.frechet_mean_ref(a, tol=1e-10)
    th = subspace_angles(a[0].astype(np.float64).T, a[1].astype(np.float64).T)      # the members' angles, by scipy on the N x k matrices themselves
    err = np.abs(info["theta"] - th[None] / 2).max()
    print("midpoint: mean-to-member angles against half the members' angles", err, "steps", info["iterations"])
    assert info["converged"] and err <= BAR
    assert abs(info["cost"][-1] - 0.5 * np.sum((th / 2) ** 2)) <= 1e-9


@pytest.mark.parametrize("k,N", [(7, 500), (17, 257)])
def test_plus_minus_pairs_have_their_base_point_as_mean(k, N):
    a, ystar = R.plus_minus_set(np.random.default_rng(3 + k), k, N)
    for m, nm in zip(a[::2], (0.3, 0.6)):                        # the construction: the largest angle of a member to Y* is ||D_j||_2
        assert abs(R.max_angle(m, ystar) - nm) <= BAR
    y, info = R.frechet_mean_ref(a, tol=1e-10)
    ang = R.max_angle(y, ystar)
    print(f"+-pairs k={k}: angle of the mean (members rounded to fp32) to Y* {ang:.2e} rad, steps {info['iterations']}")
    assert info["converged"] and ang <= BAR
    assert (np.diff(info["cost"]) <= 1e-12 * info["cost"][:-1]).all()


@pytest.mark.parametrize("k,B,N", [(1, 3, 257), (17, 5, 600)])
def test_mixing_the_rows_does_not_move_the_mean(k, B, N):
    a = R.quantised(R.clustered_set(np.random.default_rng(4 + k), B, k, N, cond=1.0))
    am = R.remix(a)
    conds = [np.linalg.cond(x.astype(np.float64) @ np.linalg.pinv(y.astype(np.float64))) for x, y in zip(am, a)]
    assert max(conds) <= 100 and (k == 1 or max(conds) > 10)
    y0, i0 = R.frechet_mean_ref(a, tol=1e-10)
    y1, i1 = R.frechet_mean_ref(am, tol=1e-10)
    ang = R.max_angle(y0, y1)
    print(f"mixing k={k}: condition numbers up to {max(conds):.1f}, angle between the means {ang:.2e} rad")
    assert ang <= BAR and np.abs(i0["theta"] - i1["theta"]).max() <= BAR and np.abs(i0["weight"] - i1["weight"]).max() <= BAR


def test_canonical_order_and_domain():
    a = R.clustered_set(np.random.default_rng(7), 5, 4, 200)
    y, info = R.frechet_mean_ref(a, tol=1e-10)
    qs = [R.orthonormal_rows(x) for x in a]
    wm = np.mean([(y @ q.T) @ (q @ y.T) for q in qs], axis=0)
    assert np.abs(wm - np.diag(info["weight"])).max() <= 1e-12 and (np.diff(info["weight"]) <= 0).all()
    assert (np.diff(info["theta"], axis=1) <= 0).all()
    q = R.random_orthonormal(np.random.default_rng(8), 6, 100)
    with pytest.raises(ValueError, match="basis 1 left the log map's domain"):
        R.frechet_mean_ref(np.stack([q[:3], q[3:]]))


def test_fixture_global_bases_are_the_restatements_means():
    """the pre-placed global bases of tests/golden/make_golden_frechet.py: orthonormal [N, 4] columns whose span has zero gradient for the four local bases"""
    f = load_golden("frechet_uncond_small.pt")
    for space, cols, stack in (("x", f["global_v"], np.stack([v.numpy() for v in f["local_vT"]])), ("h", f["global_u"], np.stack([u.numpy().T for u in f["local_u"]]))):
        y = cols.numpy().astype(np.float64).T
        assert y.shape[0] == 4 and np.abs(y @ y.T - np.eye(4)).max() <= 1e-6
        t = np.mean([R.log_map(R.orthonormal_rows(y), R.orthonormal_rows(x))[0] for x in stack], axis=0)
        print(f"space {space}: gradient norm at the fixture's basis (rounded to fp32) {np.linalg.norm(t):.2e}")
        assert np.linalg.norm(t) <= BAR


# ------------------------------------------------------------------------------------------------------------ the job and the CLI
def _driver(tmp, **kw):
    from diffusion_pullback_amd import main as m
    from diffusion_pullback_amd.edit import EditUncondDiffusion
    argv = ["--note", "t", "--model_name", "CelebA_HQ_HF", "--dataset_name", "CelebA_HQ", "--result_folder", str(tmp), "--device", "cpu",
            "--performance_boosting_t", "0.2", "--h_t", "0.8", "--edit_t", "0.6", "--seed", "0"]
    args = m.preset(m.parse_args(argv))
    args.for_steps = args.inv_steps = 20
    args.input_root = os.path.join(str(tmp), "inputs")
    for k, v in kw.items():
        setattr(args, k, v)
    return args, EditUncondDiffusion(args, unet=None)


def test_file_names_are_the_references(tmp_path):
    f = load_golden("frechet_uncond_small.pt")
    args, ed = _driver(tmp_path)
    strip = lambda d: os.path.basename(d).replace("-scheduler_yh_custom", "")      # the reference's directories carry a scheduler_name it never defines
    for space, tag in (("x", "v"), ("h", "u")):
        basis, info = ed.global_frechet_mean_paths("mid", 0, 4, 4, space)
        assert os.path.basename(os.path.dirname(basis)) == strip(f["dirs"]["glob"])
        assert os.path.basename(basis) == f"{tag}-0.8T-mid-block_0-seed_0-num_local_basis_4.pt"
        assert os.path.basename(info) == f"info-{tag}-0.8T-mid-block_0-seed_0-num_local_basis_4.pt" and os.path.dirname(info) == os.path.dirname(basis)
    own_dir, own_name = ed._tangent_space_naming("mid", 0, 4)
    assert os.path.basename(own_dir) == strip(f["dirs"]["own"]) and own_name(0, 0.8) == "xt-CelebA_HQ_0-0.8T-mid-block_0-seed_0"
    local_dir, local_name = ed._tangent_space_naming("mid", 0, 4, dataset_name="Random")       # the sampling job's files under --dataset_name Random
    assert os.path.basename(local_dir) == "local_encoder_pullback_uncond-model_CelebA_HQ_HF-dataset_Random-num_steps_20-pca_rank_4"
    assert local_name(3, 0.8) == "xt-Random_3-0.8T-mid-block_0-seed_0"
    _, ed_r = _driver(tmp_path, dataset_name="Random")
    assert ed_r._tangent_space_naming("mid", 0, 4)[0] == local_dir
    assert ed_r._tangent_space_naming("mid", 0, 4)[1](3, 0.8) == local_name(3, 0.8)


def test_argument_errors_and_the_skip_rule(tmp_path):
    f = load_golden("frechet_uncond_small.pt")
    args, ed = _driver(tmp_path)
    with pytest.raises(ValueError, match="local_projection=False is valid for frechet_mean_space 'x' only"):
        ed.run_edit_global_frechet_mean_zt(0, vis_num=4, vis_num_pc=1, pca_rank=4, num_local_basis=4, local_projection=False, frechet_mean_space="h")
    with pytest.raises(ValueError, match="frechet_mean_space must be"):
        ed.run_edit_global_frechet_mean_zt(0, vis_num=4, vis_num_pc=1, pca_rank=4, num_local_basis=4, frechet_mean_space="z")
    assert os.listdir(args.result_folder) == [] and not os.path.exists(args.input_root)
    # once the last pc's _neg picture exists nothing runs -- this driver has no U-Net, dataset or GPU to run anything with
    last = "x0_gen-" + f["runs"]["x"]["names"][-1] + ".png"
    assert last.endswith("pc_001_neg.png")
    open(os.path.join(args.result_folder, last), "w").close()
    assert ed.run_edit_global_frechet_mean_zt(0, vis_num=4, vis_pc_list=[1], pca_rank=4, num_local_basis=4, frechet_mean_space="x") is None
    assert os.listdir(args.obs_folder) == [] and os.listdir(args.result_folder) == [last] and not os.path.exists(args.input_root)
    with pytest.raises(Exception):                            # another pc is not finished (and cannot run here)
        ed.run_edit_global_frechet_mean_zt(0, vis_num=4, vis_pc_list=[0], pca_rank=4, num_local_basis=4, frechet_mean_space="x")


def test_cli_flags_parse(capsys):
    from diffusion_pullback_amd import main as m
    a = m.parse_args(["--note", "t"])
    assert a.run_edit_global_frechet_mean_zt is False and a.frechet_mean_space == "x" and (a.frechet_max_iter, a.frechet_tol) == (1000, 1e-6)
    a = m.parse_args(["--note", "t", "--run_edit_global_frechet_mean_zt", "True", "--frechet_mean_space", "h", "--num_local_basis", "100", "--model_name",
                      "CelebA_HQ_HF", "--pca_rank", "50", "--frechet_max_iter", "5000", "--frechet_tol", "1e-8"])
    assert a.run_edit_global_frechet_mean_zt is True and (a.frechet_mean_space, a.num_local_basis, a.frechet_max_iter, a.frechet_tol) == ("h", 100, 5000, 1e-8)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        m.parse_args(["--note", "t", "--run_edit_global_frechet_mean_zt", "True", "--model_name", "runwayml/stable-diffusion-v1-5"])
    err = capsys.readouterr().err
    assert "Stable Diffusion" in err and "unconditional" in err
    with pytest.raises(SystemExit):
        m.parse_args(["--note", "t", "--run_edit_global_frechet_mean_zt", "True", "--frechet_mean_space", "z"])
    with pytest.raises(SystemExit):
        m.parse_args(["--note", "t", "--run_edit_global_frechet_mean_zt", "True", "--frechet_mean_space", "h", "--local_projection", "False"])
    capsys.readouterr()
    for flag in ("--run_edit_global_frechet_mean_zt", "--frechet_mean_space", "--num_local_basis", "--frechet_max_iter", "--frechet_tol"):
        assert flag in m.__doc__


def test_engine_sizing_covers_the_local_bases_and_the_chain_call(tmp_path):
    from diffusion_pullback_amd import main as m
    argv = ["--note", "t", "--model_name", "CelebA_HQ_HF", "--dataset_name", "Random", "--result_folder", str(tmp_path), "--device", "cpu",
            "--performance_boosting_t", "0.2", "--run_edit_global_frechet_mean_zt", "True", "--num_local_basis", "100", "--pca_rank", "50"]
    a = m.preset(m.parse_args(argv))
    assert m.frechet_group(a) == 2                            # the tangent budget takes two bases of rank 50 at a time
    a.pca_rank = 10
    assert m.frechet_group(a) == 10
    a.num_local_basis = 4
    assert m.frechet_group(a) == 4


# ------------------------------------------------------------------------------------------------------------ the entry points
def _lib():
    from diffusion_pullback_amd import lib
    return lib, lib.load()


def test_symbols_are_exported_and_declared():
    lib, so = _lib()
    header = open(os.path.join(ROOT, "include", "dpb.h")).read()
    for name in ("dpb_frechet_scratch_bytes", "dpb_frechet_init", "dpb_frechet_iterate", "dpb_frechet_finish"):
        assert name in lib.SYMBOLS and getattr(so, name) is not None and name in header, name
    assert so.dpb_abi_version() == 1


def test_scratch_bytes_is_zero_for_invalid_arguments():
    _, so = _lib()
    f = so.dpb_frechet_scratch_bytes
    r = lambda b: (b + 255) // 256 * 256
    B, k, cap = 3, 5, 7
    R_ = B * k
    # status, Ghat, the whitenings, the flags, six coefficient matrices, the per-basis k x k slots, five small matrices, theta, the cost terms, the histories
    want = r(32) + r(R_ * R_ * 8) + r(B * k * k * 8) + r((2 * B + 1) * 4) + 6 * r(R_ * k * 8) + r(B * k * k * 8) + r(5 * k * k * 8) + r(R_ * 8) + r(B * 8) \
        + r((2 * cap + 1) * 8)
    assert f(B, k, 4096, cap) == want
    assert f(1, 1, 1, 0) > 0 and f(100, 50, 196608, 1000) > 8 * 5000 * 5000 and f(33, 64, 257, 10) > 0
    for b, kk, n, c in [(0, 4, 16, 10), (65536, 4, 16, 10), (2, 0, 16, 10), (2, 65, 128, 10), (2, 8, 7, 10), (2, 4, 0, 10), (2, 4, 16, -1), (-1, 4, 16, 10)]:
        assert f(b, kk, n, c) == 0, (b, kk, n, c)


def test_arguments_are_checked_before_any_gpu_call():
    lib, so = _lib()
    msg = lambda: so.dpb_last_error().decode()
    one = 256                                                    # any aligned non-null value: the checks below fail before a pointer is used
    assert so.dpb_frechet_init(None, 2, 4, 64, 0, 10, one, 1 << 30, None) != 0 and "null" in msg()
    assert so.dpb_frechet_init(one, 2, 65, 128, 0, 10, one, 1 << 30, None) != 0 and "k=65 outside [1,64]" in msg()
    assert so.dpb_frechet_init(one, 2, 4, 64, 0, 10, one + 8, 1 << 30, None) != 0 and "256-byte aligned" in msg()
    assert so.dpb_frechet_init(one, 2, 4, 64, 0, 10, one, 1024, None) != 0 and "dpb_frechet_scratch_bytes(2, 4, 64, 10)" in msg()
    assert so.dpb_frechet_init(one, 2, 4, 64, 2, 10, one, 1 << 30, None) != 0 and "init=2 outside [0,2)" in msg()
    assert so.dpb_frechet_iterate(1, 0.0, 1e-6, 2, 4, 64, 10, one, 1 << 30, None) != 0 and "step" in msg()
    assert so.dpb_frechet_iterate(-1, 1.0, 1e-6, 2, 4, 64, 10, one, 1 << 30, None) != 0 and "n_iter" in msg()
    assert so.dpb_frechet_finish(one, one, one, one, None, 2, 4, 64, 10, one, 1 << 30, None) != 0 and "null" in msg()
    from diffusion_pullback_amd import geometry
    with pytest.raises(lib.DpbError, match="HIP device"):
        geometry.frechet_mean(torch.zeros(2, 4, 64))
