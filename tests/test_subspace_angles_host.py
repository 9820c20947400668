"""CPU checks of the principal-angle / geodesic-distance feature (dpb_cross_gram, dpb_subspace_angles, geometry.py, run_tangent_space_distance): the
float64 restatement of the kernel's method against scipy.linalg.subspace_angles at the bar the GPU tests use, the new symbols and their argument
checks (which run before any GPU call), the CLI flags, and the job's refusal to run on missing files."""
import ctypes
import os

import numpy as np
import pytest

from _angles_ref import BAR, SHAPES_HOST, VARIANTS, crafted, ref_angles, scipy_angles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("k,N", SHAPES_HOST)
def test_restatement_meets_scipy_at_the_bar(k, N, variant):
    """the method itself (Gram -> row normalisation -> Cholesky whitening -> eigenvalues of I - M M^T -> asin / acos), float64, on the crafted
    inputs: <= 1e-6 rad per angle against scipy on the same fp32 inputs, small angles (0, 1e-6, 1e-4) and angles next to pi/2 included"""
    A, B = crafted(k, N, variant)
    assert np.linalg.cond(A.astype(np.float64)) < 200 and np.linalg.cond(B.astype(np.float64)) < 200      # the input domain of the bar
    theta, dist = ref_angles(A[None], B[None])
    want = scipy_angles(A, B)
    err = np.abs(theta[0, 0] - want).max()
    print(f"k={k} N={N} {variant}: worst |theta - scipy| = {err:.2e} rad")
    assert err <= BAR
    assert (np.diff(theta[0, 0]) <= 0).all()
    assert abs(dist[0, 0] - np.linalg.norm(want)) <= BAR * np.linalg.norm(want)
    if k >= 3:                                    # the crafted small angles are really there: scipy sees them
        assert abs(want[-2] - 1e-6) < 5e-7 and abs(want[-3] - 1e-4) < 5e-7


def test_restatement_self_mode_and_degenerate_rules():
    rng = np.random.default_rng(5)
    A = rng.standard_normal((4, 3, 40)).astype(np.float32)
    A[1, 2] = 0.0                                 # a zero row
    A[3, 1] = A[3, 0]                             # a duplicated row
    theta, dist = ref_angles(A)
    for i in range(4):
        for j in range(4):
            if i in (1, 3) or j in (1, 3):
                assert np.isnan(theta[i, j]).all() and np.isnan(dist[i, j])
            elif i == j:
                assert (theta[i, j] == 0).all() and dist[i, j] == 0
            else:
                assert np.array_equal(theta[i, j], theta[j, i])
                assert np.abs(theta[i, j] - scipy_angles(A[i], A[j])).max() <= BAR


def _lib():
    from diffusion_pullback_amd import lib
    return lib, lib.load()


def test_symbols_are_exported_and_declared():
    lib, so = _lib()
    header = open(os.path.join(ROOT, "include", "dpb.h")).read()
    for name in ("dpb_cross_gram", "dpb_subspace_angles", "dpb_subspace_angles_scratch_bytes"):
        assert name in lib.SYMBOLS and getattr(so, name) is not None and name in header, name
    assert so.dpb_abi_version() == 1


def test_scratch_bytes_is_zero_for_invalid_arguments():
    _, so = _lib()
    f = so.dpb_subspace_angles_scratch_bytes
    good = f(3, 2, 5, 4096)
    # the cross-Gram, two stacks of whitening matrices, the flags and the pair workgroups' slots, each rounded up to 256 bytes
    r = lambda b: (b + 255) // 256 * 256
    assert good == r(15 * 10 * 8) + r(3 * 25 * 8) + r(2 * 25 * 8) + r(5 * 4) + r(6 * 2 * 25 * 8)
    assert f(1, 1, 128, 128) > 0 and f(1, 1, 1, 1) > 0
    for ba, bb, k, n in [(1, 1, 0, 16), (1, 1, 129, 4096), (1, 1, 5, 4), (0, 1, 4, 16), (1, 0, 4, 16), (-1, 1, 4, 16), (1, 1, 4, 0), (1, 1, 4, -3),
                         (65536, 1, 4, 16)]:
        assert f(ba, bb, k, n) == 0, (ba, bb, k, n)
    assert f(100, 100, 50, 16384) >= 8 * 5000 * 5000       # the job's size: the fp64 cross-Gram of all rows dominates


def test_entry_points_refuse_bad_arguments_with_a_message():
    """every check below happens on the host, before the first launch: no GPU is needed (the pointers are never dereferenced)"""
    _, so = _lib()
    fake = ctypes.c_void_p(1 << 20)               # non-null, 256-byte aligned, never touched
    need = so.dpb_subspace_angles_scratch_bytes(2, 2, 4, 64)
    err = lambda: so.dpb_last_error().decode()
    assert so.dpb_subspace_angles(None, None, 2, 2, 4, 64, fake, fake, fake, need, None) != 0 and "null" in err()
    assert so.dpb_subspace_angles(fake, None, 2, 2, 4, 64, None, fake, fake, need, None) != 0 and "null" in err()
    assert so.dpb_subspace_angles(fake, None, 2, 2, 4, 64, fake, None, fake, need, None) != 0 and "null" in err()
    assert so.dpb_subspace_angles(fake, None, 2, 2, 4, 64, fake, fake, None, need, None) != 0 and "null" in err()
    assert so.dpb_subspace_angles(fake, None, 2, 2, 4, 64, fake, fake, fake, need - 1, None) != 0
    assert "scratch" in err() and str(need) in err()
    assert so.dpb_subspace_angles(fake, None, 2, 3, 4, 64, fake, fake, fake, 1 << 30, None) != 0 and "self mode" in err()
    assert so.dpb_subspace_angles(fake, fake, 2, 2, 129, 4096, fake, fake, fake, 1 << 30, None) != 0 and "k=129" in err()
    assert so.dpb_subspace_angles(fake, fake, 2, 2, 8, 4, fake, fake, fake, 1 << 30, None) != 0 and "N=4" in err()
    assert so.dpb_subspace_angles(fake, fake, 2, 2, 4, 64, fake, fake, ctypes.c_void_p((1 << 20) + 8), need, None) != 0 and "aligned" in err()
    assert so.dpb_cross_gram(None, None, fake, 4, 4, 16, None) != 0 and "null" in err()
    assert so.dpb_cross_gram(fake, None, None, 4, 4, 16, None) != 0 and "null" in err()
    assert so.dpb_cross_gram(fake, None, fake, 4, 5, 16, None) != 0 and "Rb = Ra" in err()
    assert so.dpb_cross_gram(fake, fake, fake, 0, 5, 16, None) != 0 and "Ra=0" in err()
    assert so.dpb_cross_gram(fake, fake, fake, 4, 5, 0, None) != 0 and "N=0" in err()


def test_geometry_refuses_cpu_tensors_and_bad_shapes():
    import torch

    from diffusion_pullback_amd import geometry
    from diffusion_pullback_amd.lib import DpbError
    with pytest.raises(DpbError, match="no CPU fallback"):
        geometry.subspace_angles(torch.zeros(2, 3, 8))
    with pytest.raises(DpbError, match="no CPU fallback"):
        geometry.cross_gram(torch.zeros(3, 8))


def test_cli_flags_parse():
    from diffusion_pullback_amd import main as m
    a = m.parse_args(["--note", "t"])
    assert a.run_tangent_space_distance is False and a.distance_space == "x"
    a = m.parse_args(["--note", "t", "--run_tangent_space_distance", "True", "--distance_space", "h", "--h_t_list", "0.8,0.5"])
    assert a.run_tangent_space_distance is True and a.distance_space == "h" and a.h_t_values == [0.8, 0.5]
    with pytest.raises(SystemExit):
        m.parse_args(["--note", "t", "--distance_space", "z"])
    assert "--run_tangent_space_distance" in m.__doc__ and "--distance_space" in m.__doc__


def _driver(tmp, kind):
    """a driver without a U-Net engine: the distance job needs the files only"""
    from diffusion_pullback_amd import main as m
    from diffusion_pullback_amd.edit import EditStableDiffusion, EditUncondDiffusion
    common = ["--note", "t", "--result_folder", str(tmp), "--device", "cpu", "--dataset_name", "Random"]
    if kind == "sd":
        argv = common + ["--model_name", "runwayml/stable-diffusion-v1-5", "--edit_prompt", "tiger", "--for_steps", "20", "--inv_steps", "20"]
    else:
        argv = common + ["--model_name", "CelebA_HQ_HF", "--performance_boosting_t", "0.2"]
    a = m.preset(m.parse_args(argv))
    a.input_root = os.path.join(str(tmp), "inputs")
    return a, (EditStableDiffusion if kind == "sd" else EditUncondDiffusion)(a, unet=None)


@pytest.mark.parametrize("kind", ["sd", "ddpm"])
def test_distance_job_lists_missing_files_and_never_samples(tmp_path, kind):
    import torch
    a, ed = _driver(tmp_path, kind)
    kw = dict(h_t=[0.8, 0.5], op="mid", block_idx=0, pca_rank=4, num_local_basis=2)
    if kind == "sd":
        d = os.path.join(a.input_root, "local_encoder_pullback_stable_diffusion-dataset_Random-num_steps_20-pca_rank_4")
        name = lambda i, ht: f'zt-Random_{i}-{ht}T-"tiger"-mid-block_0-seed_0'
    else:
        kw["fix_xt"] = True
        d = os.path.join(a.input_root, "local_encoder_pullback_uncond-model_CelebA_HQ_HF-dataset_Random-num_steps_100-pca_rank_4-fix_xt")
        name = lambda i, ht: f"xt-Random_{i}-{ht}T-mid-block_0-seed_0"
    order = [(i, ht) for ht in (0.8, 0.5) for i in range(2)]      # the order of _pending_tangent_spaces
    with pytest.raises(ValueError) as e:
        ed.run_tangent_space_distance(space="x", **kw)
    for i, ht in order:
        assert "vT-" + name(i, ht) + ".pt" in str(e.value)
    assert "sampling job" in str(e.value) and "u-" + name(0, 0.8) not in str(e.value)
    os.makedirs(d, exist_ok=True)
    for i, ht in order[:-1]:                      # all but the last are there: the message names exactly the missing one
        torch.save(torch.zeros(4, 8), os.path.join(d, "vT-" + name(i, ht) + ".pt"))
    with pytest.raises(ValueError) as e:
        ed.run_tangent_space_distance(space="x", **kw)
    assert "vT-" + name(1, 0.5) + ".pt" in str(e.value) and "vT-" + name(0, 0.8) + ".pt" not in str(e.value) and "1 of 4" in str(e.value)
    with pytest.raises(ValueError) as e:          # the h-space job looks for the u- files
        ed.run_tangent_space_distance(space="h", **kw)
    assert "u-" + name(0, 0.8) + ".pt" in str(e.value) and "4 of 4" in str(e.value)
    with pytest.raises(ValueError, match="space must be"):
        ed.run_tangent_space_distance(space="z", **kw)
    listed = ed._tangent_space_pairs([0.8, 0.5], 2, d, ed._tangent_space_naming("mid", 0, 4, **({"fix_xt": True} if kind == "ddpm" else {}))[1])
    assert [(i, ht) for i, ht, _, _ in listed] == order
    assert [(i, ht) for i, ht, _, _ in ed._pending_tangent_spaces([0.8, 0.5], 2, d, lambda i, ht: name(i, ht))] == order
