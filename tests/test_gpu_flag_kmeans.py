"""geometry.flag_kmeans (dpb_flag_kmeans_*, csrc/flagkmeans.hip) on the GPU against tests/_flag_kmeans_ref.py, the numpy float64 restatement in the
ambient space (QR per member, flag_mean_ref per cluster, ||Q Y^T||_F^2), on the same fp32 inputs.

Trajectory equality (labels after every round, moved, kept) is claimed only for the sets of _flag_kmeans_ref.TRAJECTORY_CASES, where the reference
shows in every round a relative gap >= 0.05 after row r in every cluster and a decision margin >= 1e-3 (tests/test_flag_kmeans_host.py asserts
both on the CPU); the objective then agrees within 1e-9 relative, entry by entry.  The fit checks hold on every case, at the flag mean's bars: span
within 1e-6 rad for every row count with a gap, weight and Y Y^T - I within 4 2^-24, affinities within 4 2^-24 r."""
import functools

import numpy as np
import pytest
import torch

import _flag_kmeans_ref as K
import _flag_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 1e-6
EPS = 4 * 2.0 ** -24
GAP = 0.05


def _geo():
    from diffusion_pullback_amd import geometry
    return geometry


def _dev(a):
    return torch.tensor(np.asarray(a), device=DEV)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def _trajectory(case):
    a, truth, seeds, r = K.trajectory_case(case)
    a.setflags(write=False)
    return a, truth, seeds, r, K.flag_kmeans_ref(a, len(case[0]), r, init=seeds)


def _fit_checks(a, r, labels, Y, info, what):
    """the fixed-point and fit checks: independent of how the labels were reached"""
    b, k, n = a.shape
    lab = labels.cpu().numpy()
    c = int(lab.max()) + 1
    Yn = _np(Y)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (b,) and tuple(Y.shape) == (c, r, n) and Y.dtype == torch.float32
    assert tuple(info["affinity"].shape) == (b, c) and info["affinity"].dtype == torch.float64 and tuple(info["weight"].shape) == (c, r)
    assert np.array_equal(info["sizes"], np.bincount(lab, minlength=c)) and info["sizes"].min() >= 1
    firsts = [int(np.nonzero(lab == j)[0][0]) for j in range(c)]
    assert firsts == sorted(firsts) and lab[0] == 0, f"{what}: clusters are numbered by their lowest member"
    assert info["monotone"], f"{what}: objective {info['objective']}"
    refs = [R.flag_mean_ref(a[lab == j], r) for j in range(c)]
    worst_ang = worst_w = worst_orth = 0.0
    for j, (yr, ir) in enumerate(refs):
        gaps = R.rel_gaps(ir["eigenvalues"])
        rows = [q for q in range(1, r + 1) if gaps[q - 1] >= GAP]
        worst_ang = max([worst_ang] + [R.max_angle(Yn[j][:q], yr[:q]) for q in rows])
        worst_w = max(worst_w, np.abs(_np(info["weight"][j]) - ir["weight"]).max())
        worst_orth = max(worst_orth, np.abs(Yn[j] @ Yn[j].T - np.eye(r)).max())
    aref = K.affinity_ref(a, np.stack([y for y, _ in refs]))
    got = info["affinity"].cpu().numpy()
    determined = all(R.rel_gaps(ir["eigenvalues"])[r - 1] >= GAP for _, ir in refs)
    a_err = np.abs(got - aref).max() if determined else 0.0
    again = _geo().flag_affinity(_dev(a), Y).cpu().numpy()
    a2_err = np.abs(again - got).max()
    print(f"{what}: rounds {info['rounds']}, moved {info['moved']}, kept {info['kept']}, sizes {info['sizes'].tolist()}, inner {info['inner_iterations']}; "
          f"span {worst_ang:.1e} rad, weight {worst_w:.1e}, |Y Y^T - I| {worst_orth:.1e}, affinity {a_err:.1e} (bar {EPS * r:.1e}), "
          f"flag_affinity(A, Y) against it {a2_err:.1e}")
    assert worst_ang <= BAR and worst_w <= EPS and worst_orth <= EPS, what
    assert a_err <= EPS * r and a2_err <= EPS * r, what
    if determined and c > 1:
        srt = np.sort(aref, axis=1)
        sure = (srt[:, -1] - srt[:, -2]) >= K.MIN_MARGIN
        assert np.array_equal(lab[sure], np.argmax(aref, axis=1)[sure]), what


@pytest.mark.parametrize("case", K.TRAJECTORY_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_the_trajectory_is_the_references(case):
    a, truth, seeds, r, (lab_r, y_r, ir) = _trajectory(case)
    labels, Y, info = _geo().flag_kmeans(_dev(a), len(case[0]), rank=r, init=seeds, history=True)
    rel = np.abs(info["objective"] - ir["objective"]) / ir["objective"] if len(info["objective"]) == len(ir["objective"]) else np.array([np.inf])
    print(f"{case}: moved {info['moved']} (reference {ir['moved']}), objective rel. error {rel.max():.1e}")
    assert np.array_equal(info["start"], ir["start"])
    assert len(info["history"]) == len(ir["history"]) and all(np.array_equal(x, y) for x, y in zip(info["history"], ir["history"]))
    assert info["moved"] == ir["moved"] and info["kept"] == ir["kept"] and info["rounds"] == ir["rounds"] and info["converged"]
    assert np.array_equal(labels.cpu().numpy(), lab_r) and info["seeds"] == ir["seeds"]
    assert rel.max() <= 1e-9
    assert all(info["inner_converged"])
    _fit_checks(a, r, labels, Y, info, f"{case}")


@pytest.mark.parametrize("sizes,k,n,r", [((5, 4, 3), 5, 131, 2), ((20, 13, 7), 32, 2050, 6)], ids=["5-4-3", "20-13-7"])
def test_default_seeding_recovers_well_separated_families(sizes, k, n, r):
    a, truth = K.planted_set(np.random.default_rng(7), sizes, k, n, r, 0.15)
    labels, Y, info = _geo().flag_kmeans(_dev(a), len(sizes), rank=r)
    assert K.same_partition(labels.cpu().numpy(), truth) and info["converged"] and info["rounds"] <= 2
    _fit_checks(a, r, labels, Y, info, f"planted {sizes}")


def test_one_cluster_is_the_flag_mean():
    a, _ = K.planted_set(np.random.default_rng(3), (7,), 5, 131, 3, 0.4)
    g = _geo()
    labels, Y, info = g.flag_kmeans(_dev(a), 1, rank=3)
    Ym, im = g.flag_mean(_dev(a), rank=3)
    assert (labels == 0).all() and info["rounds"] == 1 and info["moved"] == [0] and info["converged"]
    assert R.max_angle(_np(Y[0]), _np(Ym)) <= BAR and np.abs(_np(info["weight"][0]) - _np(im["weight"])).max() <= EPS
    assert abs(info["objective"][0] - 7 * (3 - float(_np(im["weight"]).sum()))) <= 7 * 3 * EPS
    _fit_checks(a, 3, labels, Y, info, "C = 1")


def test_every_member_its_own_cluster_one_member_and_full_rank():
    a, _ = K.planted_set(np.random.default_rng(4), (3, 3), 5, 67, 2, 0.5)
    g = _geo()
    labels, Y, info = g.flag_kmeans(_dev(a), 6, rank=3)                       # C = B
    assert labels.cpu().tolist() == list(range(6)) and np.abs(info["objective"]).max() <= 6 * 3 * EPS and info["sizes"].tolist() == [1] * 6
    assert np.abs(np.diag(info["affinity"].cpu().numpy()) - 3.0).max() <= 3 * EPS
    labels, Y, info = g.flag_kmeans(_dev(a[:1]), 1)                           # B = 1, rank None = k
    assert labels.cpu().tolist() == [0] and tuple(Y.shape) == (1, 5, 67) and R.max_angle(_np(Y[0]), a[0]) <= BAR
    assert abs(info["objective"][-1]) <= 5 * EPS
    labels, Y, info = g.flag_kmeans(_dev(a), 2, rank=5, init=[0, 1])          # r = k: every row sits in the bulk of 3-member clusters
    assert tuple(Y.shape) == (2, 5, 67) and info["sizes"].sum() == 6
    Yn = _np(Y)
    assert max(np.abs(Yn[j] @ Yn[j].T - np.eye(5)).max() for j in range(2)) <= EPS


def test_identical_seeds_keep_their_clusters_and_max_rounds_zero():
    a, truth = K.planted_set(np.random.default_rng(5), (4, 4), 3, 40, 2, 0.3)
    a = a.copy()
    a[1] = a[0]
    g = _geo()
    labels, Y, info = g.flag_kmeans(_dev(a), 2, rank=2, init=[0, 1], max_rounds=0)
    assert info["rounds"] == 0 and not info["converged"] and len(info["objective"]) == 1 and info["moved"] == []
    lab = labels.cpu().numpy()
    assert lab[0] == 0 and lab[1] == 1 and np.array_equal(lab, K.renumber(info["start"])[0])
    _, _, ir = K.flag_kmeans_ref(a, 2, 2, init=[0, 1], max_rounds=0)
    assert np.array_equal(info["start"], ir["start"]) and abs(info["objective"][0] - ir["objective"][0]) <= 1e-9 * ir["objective"][0]


def test_two_runs_are_bitwise_equal():
    a, truth, seeds, r, _ = _trajectory(K.TRAJECTORY_CASES[3])
    g = _geo()
    l0, y0, i0 = g.flag_kmeans(_dev(a), 4, rank=r, init=seeds)
    l1, y1, i1 = g.flag_kmeans(_dev(a), 4, rank=r, init=seeds)
    assert torch.equal(l0, l1) and torch.equal(y0, y1) and torch.equal(i0["affinity"], i1["affinity"]) and torch.equal(i0["weight"], i1["weight"])
    assert np.array_equal(i0["objective"], i1["objective"]) and i0["moved"] == i1["moved"]


def test_a_degenerate_member():
    a, truth = K.planted_set(np.random.default_rng(7), (5, 4, 3), 5, 131, 2, 0.15)
    bad = a.copy()
    bad[4, 2] = 0.0
    g = _geo()
    with pytest.raises(ValueError, match=r"indices \[4\]"):
        g.flag_kmeans(_dev(bad), 3, rank=2)
    labels, Y, info = g.flag_kmeans(_dev(bad), 3, rank=2, check=False)
    lab = labels.cpu().numpy()
    keep = np.arange(12) != 4
    assert lab[4] == -1 and info["degenerate"] == [4] and torch.isnan(info["affinity"][4]).all()
    assert K.same_partition(lab[keep], truth[keep]) and not torch.isnan(Y).any() and np.isfinite(info["objective"]).all()
    assert info["sizes"].sum() == 11


# ------------------------------------------------------------------------------------------------------------ the job, end to end
def _argv(tmp, kind, *more):
    common = ["--note", "t", "--result_folder", str(tmp), "--device", DEV, "--net_scale", "small", "--pca_rank", "3", "--num_local_basis", "4",
              "--dataset_name", "Random", *more]
    if kind == "sd":
        return common + ["--model_name", "runwayml/stable-diffusion-v1-5", "--edit_prompt", "tiger", "--for_steps", "20", "--inv_steps", "20"]
    return common + ["--model_name", "CelebA_HQ_HF", "--performance_boosting_t", "0.2"]


@pytest.mark.parametrize("kind", ["sd", "ddpm"])
def test_cluster_job_end_to_end(tmp_path, kind, monkeypatch):
    """the toy nets of tests/test_gpu_tspace.py: 4 bases at pca_rank 3 through the CLI entry, then the cluster job (C = 2, r = 2): the file's keys and
    shapes, its labels against flag_kmeans on the saved stack, the png; a deleted file makes the job raise"""
    import os
    import re

    from diffusion_pullback_amd import main as m
    root = os.path.join(str(tmp_path), "inputs")
    real_preset = m.preset

    def preset(args):                             # the drivers' basis cache goes under the test's directory
        args = real_preset(args)
        args.input_root = root
        return args
    monkeypatch.setattr(m, "preset", preset)
    m.main(_argv(tmp_path, kind, "--run_sample_encoder_local_tangent_space_zt", "True"))
    if kind == "sd":
        d = os.path.join(root, "local_encoder_pullback_stable_diffusion-dataset_Random-num_steps_20-pca_rank_3")
        name = lambda i: f'zt-Random_{i}-0.8T-"tiger"-mid-block_0-seed_0'
    else:
        d = os.path.join(root, "local_encoder_pullback_uncond-model_CelebA_HQ_HF-dataset_Random-num_steps_100-pca_rank_3")
        name = lambda i: f"xt-Random_{i}-0.8T-mid-block_0-seed_0"
    ed = m.main(_argv(tmp_path, kind, "--run_tangent_space_clusters", "True", "--num_clusters", "2", "--cluster_rank", "2"))
    out_path = os.path.join(d, ed.EXP_NAME + ".pt")
    assert os.path.basename(out_path).startswith("tangent_space_clusters-x-C2-r2-") and os.path.exists(out_path) and os.path.exists(out_path[:-3] + ".png")
    out = torch.load(out_path)
    assert set(out) == {"names", "idx", "h_t", "labels", "centres", "affinity", "objective", "weight", "gap", "sizes", "converged"}
    assert out["names"] == [name(i) for i in range(4)] and out["idx"] == [0, 1, 2, 3] and out["h_t"] == [0.8] * 4
    stack = torch.stack([torch.load(os.path.join(d, "vT-" + n + ".pt"), map_location=DEV).float() for n in out["names"]])
    n = stack.shape[2]
    assert tuple(out["labels"].shape) == (4,) and tuple(out["centres"].shape) == (2, 2, n) and tuple(out["affinity"].shape) == (4, 2)
    assert tuple(out["weight"].shape) == (2, 2) and len(out["gap"]) == 2 and int(out["sizes"].sum()) == 4
    labels, Y, info = _geo().flag_kmeans(stack, 2, rank=2)
    assert torch.equal(labels.cpu(), out["labels"]) and torch.equal(Y.cpu(), out["centres"]) and np.array_equal(info["objective"], out["objective"].numpy())
    os.remove(os.path.join(d, "vT-" + name(3) + ".pt"))
    with pytest.raises(ValueError, match=re.escape("vT-" + name(3) + ".pt")):
        m.main(_argv(tmp_path, kind, "--run_tangent_space_clusters", "True", "--num_clusters", "2", "--cluster_rank", "2"))
