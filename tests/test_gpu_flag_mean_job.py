"""EditUncondDiffusion.run_edit_global_flag_mean_zt on the HIP engine, on the toy DDPM net and the four pre-placed local bases of
tests/test_gpu_frechet_job.py's fixture: the files it writes ([N, r] columns, the info keys), the basis against tests/_flag_ref.py, the load branch of
a second call, a flag_rank below pca_rank, the pc range -- and the Frechet job started at the flag mean (--frechet_init flag)."""
import os

import numpy as np
import pytest
import torch

import _flag_ref as R
from _util import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def fix():
    return load_golden("frechet_uncond_small.pt")


def _driver(f, tmp, extra=()):
    """the fixture's toy net behind a driver whose local bases (and the sample's own) are in place"""
    from diffusion_pullback_amd import PullbackUNet, configs as cf
    from diffusion_pullback_amd import edit as E
    from diffusion_pullback_amd import main as m
    from oracle import unet_ddpm
    a = f["args"]
    cfg = unet_ddpm.DDPMConfig(**f["cfg"])
    params = cf.ddpm_init_params(cfg, seed=f["seed"], spectrum=cf.Spectrum(**f["spectrum"]))
    net = PullbackUNet("ddpm", cfg, params, dtype=torch.float32, device=DEV, max_batch=20, max_rank=4, verbose=False)
    argv = ["--note", "t", "--model_name", a["model_name"], "--dataset_name", a["dataset_name"], "--result_folder", str(tmp), "--device", DEV,
            "--performance_boosting_t", "0.2", "--x_space_guidance_edit_step", str(a["x_space_guidance_edit_step"]), "--x_space_guidance_scale",
            str(a["x_space_guidance_scale"]), "--x_space_guidance_num_step", str(a["x_space_guidance_num_step"]), "--edit_t", str(a["edit_t"]),
            "--h_t", str(a["h_t"]), "--seed", str(a["seed"]), "--trajectory_batch", "20", *extra]
    args = m.preset(m.parse_args(argv))
    args.for_steps = args.inv_steps = a["for_steps"]
    args.image_size = 32
    args.input_root = os.path.join(str(tmp), "inputs")
    ed = E.EditUncondDiffusion(args, unet=net, dataset={0: f["x0"]})
    ed.performance_boosting_t_idx = 1000
    k, n = a["pca_rank"], a["num_local_basis"]
    local_dir, local_name = ed._tangent_space_naming("mid", 0, k, dataset_name="Random")
    own_dir, own_name = ed._tangent_space_naming("mid", 0, k)
    os.makedirs(local_dir, exist_ok=True); os.makedirs(own_dir, exist_ok=True)
    for i in range(n):
        torch.save(f["local_u"][i], os.path.join(local_dir, f"u-{local_name(i, a['h_t'])}.pt"))
        torch.save(f["local_vT"][i], os.path.join(local_dir, f"vT-{local_name(i, a['h_t'])}.pt"))
    torch.save(f["own_u"], os.path.join(own_dir, f"u-{own_name(0, a['h_t'])}.pt"))
    torch.save(f["own_vT"], os.path.join(own_dir, f"vT-{own_name(0, a['h_t'])}.pt"))
    return args, ed


def _job(ed, f, monkeypatch, **kw):
    from diffusion_pullback_amd import edit as E
    a = f["args"]
    saved = []
    monkeypatch.setattr(E, "save_image", lambda x, path, nrow=None: saved.append(os.path.basename(path)))
    torch.manual_seed(a["rng_seed"])
    out = ed.run_edit_global_flag_mean_zt(a["idx"], op="mid", block_idx=0, vis_num=a["vis_num"], pca_rank=a["pca_rank"],
                                          num_local_basis=a["num_local_basis"], **kw)
    return out, saved


@pytest.mark.parametrize("space,rank", [("x", None), ("h", 2)])
def test_the_job_writes_loads_and_edits(fix, tmp_path, monkeypatch, capsys, space, rank):
    a = fix["args"]
    k, n = a["pca_rank"], a["num_local_basis"]
    r = k if rank is None else rank
    args, ed = _driver(fix, tmp_path)
    out, saved = _job(ed, fix, monkeypatch, flag_mean_space=space, flag_rank=rank, vis_pc_list=[r - 1])
    basis_path, info_path = ed.global_flag_mean_paths("mid", 0, k, n, space, flag_rank=rank)
    assert os.path.basename(basis_path) == f"{'v' if space == 'x' else 'u'}-{a['h_t']}T-mid-block_0-seed_{a['seed']}-num_local_basis_{n}-rank_{r}.pt"
    stack = np.stack([v.numpy() for v in fix["local_vT"]]) if space == "x" else np.stack([u.numpy().T for u in fix["local_u"]])
    cols, info = torch.load(basis_path), torch.load(info_path, weights_only=False)
    assert tuple(cols.shape) == (stack.shape[2], r) and cols.dtype == torch.float32
    assert set(info) >= {"weight", "eigenvalues", "gap", "theta", "iterations", "converged", "residual", "degenerate", "space", "names"}
    assert info["space"] == space and len(info["names"]) == n and tuple(info["theta"].shape) == (n, r) and tuple(info["weight"].shape) == (r,)
    Yr, ir = R.flag_mean_ref(stack, r)
    w_err = np.abs(info["weight"].numpy() - ir["weight"]).max()
    gaps = R.rel_gaps(ir["eigenvalues"])
    print(f"space {space} rank {r}: weights {np.round(ir['eigenvalues'][:r + 2], 4)}, weight error {w_err:.2e}, converged {info['converged']}")
    assert w_err <= 4 * 2.0 ** -24
    if gaps[r - 1] >= 0.05:
        assert info["converged"] and R.max_angle(cols.numpy().T, Yr) <= 1e-6
    assert "flag mean of 4 local bases" in capsys.readouterr().out
    assert tuple(out["basis"].shape) == (r, stack.shape[2]) and tuple(out["vk"].shape)[0] == 1 and out["info"] is not None
    assert len(out["names"]) == 2 and sorted(x for x in saved if x.startswith("x0_gen-")) == sorted(f"x0_gen-{x}.png" for x in out["names"])
    # a second call loads the file: same rows (column-normalised), no info
    again, _ = _job(ed, fix, monkeypatch, flag_mean_space=space, flag_rank=rank, vis_pc_list=[])
    assert again["info"] is None and torch.allclose(again["basis"].cpu(), out["basis"].cpu(), atol=1e-6)
    with pytest.raises(ValueError, match=f"{r} rows"):
        _job(ed, fix, monkeypatch, flag_mean_space=space, flag_rank=rank, vis_pc_list=[r])


def test_frechet_job_started_at_the_flag_mean(fix, tmp_path, monkeypatch):
    from diffusion_pullback_amd import edit as E
    a = fix["args"]
    k, n = a["pca_rank"], a["num_local_basis"]
    args, ed = _driver(fix, tmp_path)
    monkeypatch.setattr(E, "save_image", lambda x, path, nrow=None: None)
    torch.manual_seed(a["rng_seed"])
    out = ed.run_edit_global_frechet_mean_zt(a["idx"], vis_num=a["vis_num"], vis_pc_list=[], pca_rank=k, num_local_basis=n, frechet_mean_space="x",
                                             frechet_tol=1e-10, frechet_init="flag")
    basis_path, info_path = ed.global_frechet_mean_paths("mid", 0, k, n, "x")
    info = torch.load(info_path, weights_only=False)
    assert info["init"] == "flag" and info["converged"] and info["flag_converged"] and info["flag_iterations"] >= 1
    want = fix["global_v"]
    ang = R.max_angle(torch.load(basis_path).numpy().T, want.numpy().T)
    print(f"Frechet job from the flag mean: {info['iterations']} steps, {ang:.2e} rad from the fixture's mean")
    assert ang <= 1e-6


def test_cli_end_to_end_on_synthetic_weights(tmp_path, monkeypatch):
    """--run_edit_global_flag_mean_zt True --flag_rank 2 --pca_rank 3 --num_local_basis 8 --net_scale small: the engine sized by main.build_unet, the
    local bases sampled in groups, the v- file of two columns, the info file and the pictures"""
    from diffusion_pullback_amd import main as m
    monkeypatch.chdir(tmp_path)
    preset = m.preset

    def short(args):
        args = preset(args)
        args.for_steps = args.inv_steps = 20
        return args
    monkeypatch.setattr(m, "preset", short)
    argv = ["--note", "t", "--model_name", "CelebA_HQ_HF", "--dataset_name", "Random", "--result_folder", str(tmp_path / "runs"), "--device", DEV,
            "--net_scale", "small", "--performance_boosting_t", "0.2", "--x_space_guidance_scale", "0.1", "--x_space_guidance_num_step", "4",
            "--edit_t", "0.6", "--h_t", "0.8", "--run_edit_global_flag_mean_zt", "True", "--flag_mean_space", "x", "--flag_rank", "2",
            "--num_local_basis", "8", "--pca_rank", "3", "--vis_num_pc", "1"]
    ed = m.main(argv)
    assert ed.unet.engine.max_batch >= 8 and ed.unet.max_rank >= 24
    basis_path, info_path = ed.global_flag_mean_paths("mid", 0, 3, 8, "x", flag_rank=2)
    assert os.path.basename(basis_path) == "v-0.8T-mid-block_0-seed_0-num_local_basis_8-rank_2.pt"
    cols, info = torch.load(basis_path), torch.load(info_path, weights_only=False)
    assert tuple(cols.shape) == (3 * 32 * 32, 2) and torch.isfinite(cols).all()
    assert torch.allclose(cols.t() @ cols, torch.eye(2), atol=1e-5)
    assert len(info["names"]) == 8 and len(info["eigenvalues"]) == 16 and (np.diff(info["eigenvalues"]) <= 1e-12).all()
    stem = "x0_gen-xt-Random_0-h_0.8T-edit_0.6T-mid-block_0-seed_0-pc_000_"
    assert sorted(x for x in os.listdir(ed.result_folder) if x.startswith("x0_gen-")) == [stem + "neg.png", stem + "pos.png"]
