"""CPU-only checks of flag k-means and the chordal affinity: the numpy reference (tests/_flag_kmeans_ref.py) against itself and against constructions,
the conditions under which tests/test_gpu_flag_kmeans.py claims trajectory equality, the ABI surface, the argument checks (which run before any GPU
call), the CLI flags, and the job's file names and its refusal to run on missing files."""
import ctypes
import functools
import os

import numpy as np
import pytest
from scipy.linalg import subspace_angles

import _flag_kmeans_ref as K
import _flag_ref as R
from _frechet_ref import random_orthonormal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dpb_flag_affinity_scratch_bytes", "dpb_flag_affinity", "dpb_flag_kmeans_scratch_bytes", "dpb_flag_kmeans_host_bytes", "dpb_flag_kmeans_affinity",
         "dpb_flag_kmeans_init", "dpb_flag_kmeans_gather", "dpb_flag_kmeans_set_centre", "dpb_flag_kmeans_assign", "dpb_flag_kmeans_finish")


# ------------------------------------------------------------------------------------------------------------ the reference
def test_affinity_is_the_sum_of_squared_cosines_for_unequal_ranks():
    rng = np.random.default_rng(0)
    for k, r, n in [(5, 2, 40), (3, 7, 40), (4, 4, 9), (1, 6, 17)]:
        a, y = rng.standard_normal((k, n)), rng.standard_normal((r, n))
        want = np.sum(np.cos(subspace_angles(a.T, y.T)) ** 2)
        got = K.affinity_ref(a[None], y[None])[0, 0]
        assert abs(got - want) <= 1e-12 and -1e-12 <= got <= min(k, r) + 1e-12


@pytest.mark.parametrize("sizes,k,n,r", [((5, 4, 3), 5, 131, 2), ((6, 6), 4, 40, 3)])
def test_planted_sets_are_recovered_and_the_objective_does_not_rise(sizes, k, n, r):
    a, truth = K.planted_set(np.random.default_rng(7), sizes, k, n, r, 0.15)
    labels, y, info = K.flag_kmeans_ref(a, len(sizes), r)
    assert K.same_partition(labels, truth) and info["converged"] and info["rounds"] <= 2
    assert labels[0] == 0 and np.array_equal(info["sizes"], np.bincount(labels))
    a, truth, seeds, r = K.trajectory_case(K.TRAJECTORY_CASES[3])
    _, _, info = K.flag_kmeans_ref(a, 4, r, init=seeds)
    assert len(info["objective"]) == info["rounds"] and (np.diff(info["objective"]) <= 1e-12).all()


def test_one_cluster_is_the_flag_mean_and_one_cluster_each_costs_nothing():
    a, _ = K.planted_set(np.random.default_rng(3), (7,), 5, 131, 3, 0.4)
    labels, y, info = K.flag_kmeans_ref(a, 1, 3)
    yr, ir = R.flag_mean_ref(a, 3)
    assert (labels == 0).all() and R.max_angle(y[0], yr) <= 1e-12 and np.allclose(info["weight"][0], ir["weight"], atol=1e-14)
    assert abs(info["objective"][0] - 7 * (3 - ir["weight"].sum())) <= 1e-12 and info["moved"] == [0]
    labels, y, info = K.flag_kmeans_ref(a, 7, 3)
    assert labels.tolist() == list(range(7)) and np.abs(info["objective"]).max() <= 1e-12
    _, _, info0 = K.flag_kmeans_ref(a, 2, 3, init=[0, 1], max_rounds=0)
    assert info0["rounds"] == 0 and len(info0["objective"]) == 1 and not info0["converged"]


def test_seeding_is_farthest_first_and_seeds_keep_their_clusters():
    f = random_orthonormal(np.random.default_rng(1), 8, 30)
    qs = [f[0:2], f[0:2], np.stack([f[0], f[2]]), f[4:6]]              # members 0 and 1 identical, 2 shares a row, 3 is orthogonal
    seeds, labels = K.seeds_ref(qs, 3, 0)
    assert seeds == [0, 3, 2] and labels.tolist() == [0, 0, 2, 1]
    seeds, labels = K.seeds_ref(qs, 2, [0, 1])
    assert labels.tolist()[:2] == [0, 1]                               # two identical members given as two seeds keep their clusters


@functools.lru_cache(maxsize=None)
def _run(case):
    a, truth, seeds, r = K.trajectory_case(case)
    return truth, K.flag_kmeans_ref(a, len(case[0]), r, init=seeds)


@pytest.mark.parametrize("case", K.TRAJECTORY_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_the_trajectory_cases_meet_their_conditions(case):
    """what lets the GPU test claim trajectory equality: in EVERY round a relative gap >= 0.05 after row r in every cluster, a decision margin >= 1e-3 for
    every member, every seed inside one planted family and at least one round that moves members"""
    truth, (labels, y, info) = _run(case)
    print(case, info["moved"], min(info["margin"]), min(info["gap"]))
    assert min(info["gap"]) >= K.MIN_GAP and min(info["margin"]) >= K.MIN_MARGIN
    assert info["converged"] and sum(info["moved"]) > 0 and len(info["moved"]) >= 2
    assert len(set(truth[info["seeds"]].tolist())) == 1
    assert (np.diff(info["objective"]) <= 0).all()


# ------------------------------------------------------------------------------------------------------------ the ABI
def _lib():
    from diffusion_pullback_amd import lib
    return lib, lib.load()


def test_symbols_are_exported_and_declared():
    lib, so = _lib()
    header = open(os.path.join(ROOT, "include", "dpb.h")).read()
    for name in NAMES:
        assert name in lib.SYMBOLS and getattr(so, name) is not None and name + "(" in header, name


def test_scratch_bytes_limits():
    _, so = _lib()
    f, g, h = so.dpb_flag_affinity_scratch_bytes, so.dpb_flag_kmeans_scratch_bytes, so.dpb_flag_kmeans_host_bytes
    r = lambda b: (b + 255) // 256 * 256
    assert f(3, 5, 2, 7, 40) == r(15 * 14 * 8) + r(3 * 25 * 8) + r(2 * 49 * 8) + r(5 * 4)
    assert f(1, 64, 1, 64, 64) > 0 and f(1, 1, 1, 1, 1) > 0
    for b, k, c, rr, n in [(0, 4, 1, 4, 16), (1, 0, 1, 4, 16), (1, 65, 1, 4, 128), (1, 4, 0, 4, 16), (1, 4, 1, 0, 16), (1, 4, 1, 65, 128), (1, 4, 1, 4, 3),
                           (1, 2, 1, 4, 3), (65536, 4, 1, 4, 16), (1, 4, 65536, 4, 16), (1, 4, 1, 4, 0)]:
        assert f(b, k, c, rr, n) == 0, (b, k, c, rr, n)
    assert h(12, 3, 24, 3, 2) == 32 + 4 * (3 * 3 + 2 * 12)
    assert g(100, 50, 16384, 4, 10) >= 8 * 5000 * 5000 + 8 * 5000 * 40 and g(1, 1, 1, 1, 1) > 0
    for b, k, n, c, rr in [(0, 4, 16, 1, 2), (4, 0, 16, 1, 1), (4, 65, 128, 1, 2), (4, 4, 3, 1, 2), (4, 4, 16, 0, 2), (4, 4, 16, 5, 2), (4, 4, 16, 2, 0),
                           (4, 4, 16, 2, 5), (65536, 4, 16, 2, 2), (32768, 64, 64, 2, 2)]:
        assert g(b, k, n, c, rr) == 0 and h(b, k, n, c, rr) == 0, (b, k, n, c, rr)


def test_entry_points_refuse_bad_arguments_with_a_message():
    """every check below happens on the host, before the first launch: no GPU is needed (the pointers are never dereferenced)"""
    _, so = _lib()
    fake = ctypes.c_void_p(1 << 20)               # non-null, 256-byte aligned, never touched
    odd = ctypes.c_void_p((1 << 20) + 8)
    err = lambda: so.dpb_last_error().decode()
    need = so.dpb_flag_affinity_scratch_bytes(3, 5, 2, 7, 40)
    assert so.dpb_flag_affinity(None, fake, 3, 5, 2, 7, 40, fake, fake, need, None) != 0 and "null" in err()
    assert so.dpb_flag_affinity(fake, fake, 3, 5, 2, 7, 40, None, fake, need, None) != 0 and "null" in err()
    assert so.dpb_flag_affinity(fake, fake, 3, 65, 2, 7, 128, fake, fake, 1 << 30, None) != 0 and "k=65" in err() and "[1,64]" in err()
    assert so.dpb_flag_affinity(fake, fake, 3, 5, 2, 7, 6, fake, fake, 1 << 30, None) != 0 and "N=6" in err()
    assert so.dpb_flag_affinity(fake, fake, 3, 5, 2, 7, 40, fake, fake, need - 1, None) != 0
    assert "dpb_flag_affinity_scratch_bytes(3, 5, 2, 7, 40)" in err() and str(need) in err()
    assert so.dpb_flag_affinity(fake, fake, 3, 5, 2, 7, 40, fake, odd, need, None) != 0 and "aligned" in err()
    need = so.dpb_flag_kmeans_scratch_bytes(12, 3, 24, 3, 2)
    seeds = (ctypes.c_int32 * 3)(0, 1, 2)
    a = (12, 3, 24, 3, 2)
    assert so.dpb_flag_kmeans_init(None, *a, seeds, 3, fake, need, None) != 0 and "null" in err()
    assert so.dpb_flag_kmeans_init(fake, *a, None, 3, fake, need, None) != 0 and "null" in err()
    assert so.dpb_flag_kmeans_init(fake, 12, 3, 24, 13, 2, seeds, 3, fake, 1 << 30, None) != 0 and "C=13" in err()
    assert so.dpb_flag_kmeans_init(fake, 12, 3, 24, 3, 4, seeds, 3, fake, 1 << 30, None) != 0 and "r=4" in err()
    assert so.dpb_flag_kmeans_init(fake, *a, seeds, 2, fake, need, None) != 0 and "n_seeds=2" in err()
    assert so.dpb_flag_kmeans_init(fake, *a, (ctypes.c_int32 * 3)(0, 12, 2), 3, fake, need, None) != 0 and "seeds[1]=12" in err()
    assert so.dpb_flag_kmeans_init(fake, *a, (ctypes.c_int32 * 3)(0, 2, 2), 3, fake, need, None) != 0 and "distinct" in err()
    assert so.dpb_flag_kmeans_init(fake, *a, seeds, 3, fake, need - 1, None) != 0
    assert "dpb_flag_kmeans_scratch_bytes(12, 3, 24, 3, 2)" in err() and str(need) in err()
    assert so.dpb_flag_kmeans_init(fake, *a, seeds, 3, odd, need, None) != 0 and "aligned" in err()
    assert so.dpb_flag_kmeans_gather(3, 4, fake, *a, fake, need, None) != 0 and "c=3" in err()
    assert so.dpb_flag_kmeans_gather(0, 0, fake, *a, fake, need, None) != 0 and "n_c=0" in err()
    assert so.dpb_flag_kmeans_gather(0, 4, odd, *a, fake, need, None) != 0 and "32-byte aligned" in err()
    assert so.dpb_flag_kmeans_gather(0, 4, None, *a, fake, need, None) != 0 and "null" in err()
    assert so.dpb_flag_kmeans_set_centre(-1, 4, fake, *a, fake, need, None) != 0 and "c=-1" in err()
    assert so.dpb_flag_kmeans_set_centre(0, 4, None, *a, fake, need, None) != 0 and "null" in err()
    assert so.dpb_flag_kmeans_assign(1, *a, None, need, None) != 0 and "null" in err()
    assert so.dpb_flag_kmeans_assign(1, *a, fake, need - 1, None) != 0 and "scratch" in err()
    assert so.dpb_flag_kmeans_finish(fake, None, *a, fake, need, None) != 0 and "null" in err()
    assert so.dpb_flag_kmeans_finish(fake, fake, 12, 3, 2, 3, 2, fake, 1 << 30, None) != 0 and "N=2" in err()
    assert not so.dpb_flag_kmeans_affinity(12, 3, 24, 13, 2, fake) and "C=13" in err()
    assert so.dpb_flag_kmeans_affinity(*a, fake) > (1 << 20)


def test_geometry_refuses_cpu_tensors_and_bad_arguments():
    import torch

    from diffusion_pullback_amd import geometry
    from diffusion_pullback_amd.lib import DpbError
    with pytest.raises(DpbError, match="no CPU fallback"):
        geometry.flag_affinity(torch.zeros(2, 3, 8), torch.zeros(1, 2, 8))
    with pytest.raises(DpbError, match="no CPU fallback"):
        geometry.flag_kmeans(torch.zeros(4, 3, 8), 2)

    class OnDevice(torch.Tensor):                 # passes the device check; the argument checks come before any GPU call
        is_cuda = True
    a = torch.zeros(4, 3, 8).as_subclass(OnDevice)
    for kw, msg in [(dict(n_clusters=0), "n_clusters = 0"), (dict(n_clusters=5), "n_clusters = 5"), (dict(n_clusters=2, rank=0), "rank = 0"),
                    (dict(n_clusters=2, rank=4), "rank = 4"), (dict(n_clusters=2, init=4), "init = 4"), (dict(n_clusters=2, init=[0]), "init must be"),
                    (dict(n_clusters=2, init=[1, 1]), "init must be"), (dict(n_clusters=2, init=[0, 4]), "init must be"),
                    (dict(n_clusters=2, max_rounds=-1), "max_rounds = -1")]:
        with pytest.raises(ValueError, match=msg):
            geometry.flag_kmeans(a, **kw)
    with pytest.raises(ValueError, match="N = 8, Y of N = 9"):
        geometry.flag_affinity(a, torch.zeros(1, 2, 9).as_subclass(OnDevice))
    with pytest.raises(ValueError, match="exceeds the rank 64"):
        geometry.flag_affinity(torch.zeros(1, 65, 80).as_subclass(OnDevice), torch.zeros(1, 2, 80).as_subclass(OnDevice))


# ------------------------------------------------------------------------------------------------------------ the CLI and the job
def test_cli_flags_parse_and_are_refused():
    from diffusion_pullback_amd import main as m
    a = m.parse_args(["--note", "t"])
    assert a.run_tangent_space_clusters is False and a.num_clusters == 2 and a.cluster_rank == 0
    a = m.parse_args(["--note", "t", "--run_tangent_space_clusters", "True", "--num_clusters", "3", "--cluster_rank", "2", "--pca_rank", "4",
                      "--num_local_basis", "2", "--h_t_list", "0.8,0.5", "--distance_space", "h"])
    assert a.run_tangent_space_clusters is True and a.num_clusters == 3 and a.cluster_rank == 2 and a.distance_space == "h"
    base = ["--note", "t", "--run_tangent_space_clusters", "True", "--pca_rank", "4", "--num_local_basis", "2", "--h_t_list", "0.8,0.5"]
    for more in (["--num_clusters", "0"], ["--num_clusters", "5"], ["--cluster_rank", "5"], ["--cluster_rank", "-1"]):
        with pytest.raises(SystemExit):
            m.parse_args(base + more)
    m.parse_args(base + ["--num_clusters", "4", "--cluster_rank", "4"])
    m.parse_args(["--note", "t", "--num_clusters", "0"])                  # (checked only when the job is asked for)
    for flag in ("--run_tangent_space_clusters", "--num_clusters", "--cluster_rank"):
        assert flag in m.__doc__


def _driver(tmp, kind):
    """a driver without a U-Net engine: the cluster job needs the files only"""
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
def test_cluster_job_names_its_files_lists_missing_ones_and_never_samples(tmp_path, kind, monkeypatch):
    import torch

    from diffusion_pullback_amd import geometry
    a, ed = _driver(tmp_path, kind)
    kw = dict(h_t=[0.8, 0.5], op="mid", block_idx=0, pca_rank=4, num_local_basis=2, num_clusters=2, cluster_rank=3)
    if kind == "sd":
        d = os.path.join(a.input_root, "local_encoder_pullback_stable_diffusion-dataset_Random-num_steps_20-pca_rank_4")
        name = lambda i, ht: f'zt-Random_{i}-{ht}T-"tiger"-mid-block_0-seed_0'
    else:
        kw["fix_xt"] = True
        d = os.path.join(a.input_root, "local_encoder_pullback_uncond-model_CelebA_HQ_HF-dataset_Random-num_steps_100-pca_rank_4-fix_xt")
        name = lambda i, ht: f"xt-Random_{i}-{ht}T-mid-block_0-seed_0"
    order = [(i, ht) for ht in (0.8, 0.5) for i in range(2)]      # the order of the sampling job
    with pytest.raises(ValueError) as e:
        ed.run_tangent_space_clusters(space="x", **kw)
    assert all("vT-" + name(i, ht) + ".pt" in str(e.value) for i, ht in order) and "sampling job" in str(e.value) and "4 of 4" in str(e.value)
    os.makedirs(d, exist_ok=True)
    for i, ht in order[:-1]:
        torch.save(torch.zeros(4, 8), os.path.join(d, "vT-" + name(i, ht) + ".pt"))
    with pytest.raises(ValueError) as e:
        ed.run_tangent_space_clusters(space="x", **kw)
    assert "vT-" + name(1, 0.5) + ".pt" in str(e.value) and "vT-" + name(0, 0.8) + ".pt" not in str(e.value) and "1 of 4" in str(e.value)
    with pytest.raises(ValueError) as e:          # the h-space job looks for the u- files
        ed.run_tangent_space_clusters(space="h", **kw)
    assert "u-" + name(0, 0.8) + ".pt" in str(e.value)
    with pytest.raises(ValueError, match="space must be"):
        ed.run_tangent_space_clusters(space="z", **kw)
    # the file names, with the clustering itself stubbed out (it needs a GPU): C, r and the set's EXP_NAME
    torch.save(torch.zeros(4, 8), os.path.join(d, "vT-" + name(1, 0.5) + ".pt"))
    seen = {}

    def stub(stack, n_clusters, rank=None, max_bytes=None):
        seen.update(shape=tuple(stack.shape), c=n_clusters, r=rank)
        info = {"affinity": torch.zeros(4, 2, dtype=torch.float64), "objective": np.zeros(1), "weight": torch.zeros(2, rank), "gap": [None, None],
                "sizes": np.array([2, 2]), "converged": True, "eigenvalues": [np.ones(4), np.ones(4)]}
        return torch.tensor([0, 1, 0, 1], dtype=torch.int32), torch.zeros(2, rank, 8), info
    monkeypatch.setattr(geometry, "flag_kmeans", stub)
    out = ed.run_tangent_space_clusters(space="x", **kw)
    assert seen == {"shape": (4, 4, 8), "c": 2, "r": 3}
    tail = name("0to1", "0.8,0.5")
    assert ed.EXP_NAME == "tangent_space_clusters-x-C2-r3-" + tail and os.path.exists(os.path.join(d, ed.EXP_NAME + ".pt"))
    assert out["names"] == [name(i, ht) for i, ht in order] and set(out) == {"names", "idx", "h_t", "labels", "centres", "affinity", "objective",
                                                                              "weight", "gap", "sizes", "converged"}
    kw["cluster_rank"] = None                     # None: pca_rank
    ed.run_tangent_space_clusters(space="x", **kw)
    assert ed.EXP_NAME == "tangent_space_clusters-x-C2-r4-" + tail
