"""EditUncondDiffusion.run_edit_global_flag_mean_zt(flag_mean_kind="median") on the HIP engine, on the toy DDPM net and the four pre-placed local
bases of tests/test_gpu_frechet_job.py's fixture: the -median files it writes ([N, r] columns, the info keys), the basis against
tests/_flag_median_ref.py, the load branch of a second call, and the mean job's files of the same directory left as they were."""
import os

import numpy as np
import pytest
import torch

import _flag_median_ref as M
import _flag_ref as R
from test_gpu_flag_mean_job import _driver, _job
from _util import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fix():
    return load_golden("frechet_uncond_small.pt")


def test_the_median_job_writes_loads_and_leaves_the_mean_alone(fix, tmp_path, monkeypatch, capsys):
    a = fix["args"]
    k, n, r = a["pca_rank"], a["num_local_basis"], 2
    args, ed = _driver(fix, tmp_path)
    _job(ed, fix, monkeypatch, flag_mean_space="x", flag_rank=r, vis_pc_list=[])
    mean_paths = ed.global_flag_mean_paths("mid", 0, k, n, "x", flag_rank=r)
    before = [open(p, "rb").read() for p in mean_paths]
    capsys.readouterr()
    out, saved = _job(ed, fix, monkeypatch, flag_mean_space="x", flag_rank=r, vis_pc_list=[r - 1], flag_mean_kind="median")
    basis_path, info_path = ed.global_flag_mean_paths("mid", 0, k, n, "x", flag_rank=r, flag_mean_kind="median")
    assert os.path.basename(basis_path) == f"v-{a['h_t']}T-mid-block_0-seed_{a['seed']}-num_local_basis_{n}-rank_{r}-median.pt"
    assert os.path.dirname(basis_path) == os.path.dirname(mean_paths[0])
    stack = np.stack([v.numpy() for v in fix["local_vT"]])
    cols, info = torch.load(basis_path), torch.load(info_path, weights_only=False)
    assert tuple(cols.shape) == (stack.shape[2], r) and cols.dtype == torch.float32
    assert set(info) >= {"weight", "eigenvalues", "gap", "theta", "converged", "degenerate", "space", "names", "member_weight", "distance", "objective",
                         "rounds", "monotone", "affinity", "inner_iterations", "inner_converged"}
    assert info["space"] == "x" and len(info["names"]) == n and tuple(info["member_weight"].shape) == (n,) and tuple(info["distance"].shape) == (n,)
    Yr, ir = M.flag_median_ref(stack, r)
    text = capsys.readouterr().out
    print(f"median job: rounds {info['rounds']} (reference {ir['rounds']}), objective {info['objective']}, min gap {ir['gaps'].min():.3f}, "
          f"min d {ir['dmin'].min():.3g}")
    assert "flag median of 4 local bases" in text and "lowest member weights" in text
    assert all(name in text for name in np.array(info["names"])[np.argsort(info["member_weight"].numpy(), kind="stable")[:5]])
    assert info["monotone"] and len(info["objective"]) == info["rounds"] + 1
    assert abs(info["objective"][0] - ir["objective"][0]) <= 1e-9 * ir["objective"][0]          # round 0 is the flag mean: no condition needed
    if M.qualifies(ir) and ir["converged"]:
        assert info["rounds"] == ir["rounds"] and info["converged"]
        assert (np.abs(info["objective"] - ir["objective"]) / ir["objective"]).max() <= 1e-9
        assert R.max_angle(cols.numpy().T, Yr) <= 1e-6
        assert (np.abs(info["member_weight"].numpy() - ir["member_weight"]) / ir["member_weight"]).max() <= 1e-8
    assert tuple(out["basis"].shape) == (r, stack.shape[2]) and tuple(out["vk"].shape)[0] == 1 and out["info"] is not None
    assert len(out["names"]) == 2 and sorted(x for x in saved if x.startswith("x0_gen-")) == sorted(f"x0_gen-{x}.png" for x in out["names"])
    # a second call loads the file: same rows (column-normalised), no info
    again, _ = _job(ed, fix, monkeypatch, flag_mean_space="x", flag_rank=r, vis_pc_list=[], flag_mean_kind="median")
    assert again["info"] is None and torch.allclose(again["basis"].cpu(), out["basis"].cpu(), atol=1e-6)
    assert [open(p, "rb").read() for p in mean_paths] == before
