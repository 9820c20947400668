"""The h-space guidance edit (--edit_ht h_space_guidance) of the global-basis jobs on the HIP engine, on the toy net, sample and pre-placed bases of
tests/test_gpu_parallel_h_job.py's fixture: the pictures and hguide-<name>.pt records under the parallel-x names, row 0 of every experiment against
the plain DDIM steps over the guided interval (relative error < 2e-3, the bar tests/test_gpu_edit.py holds batched trajectories to against one at a
time), the skip rule, chains together against one experiment after another, the other two jobs through the same tail, and the CLI end to end."""
import os

import pytest
import torch

from _util import load_golden, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-3
STEP = 20.0


@pytest.fixture(scope="module")
def fix():
    f = load_golden("parallel_h_uncond_small.pt")
    f["bases"] = load_golden("frechet_uncond_small.pt")            # the pre-placed bases, the sample and the toy net
    return f


def _run(f, tmp, trajectory_batch=20, job="frechet", mode="asyrp", local_projection=False, extra=()):
    """one run of a global-basis job in h_space_guidance mode.  Returns (save_image calls, return value, driver)."""
    from diffusion_pullback_amd import PullbackUNet, configs as cf
    from diffusion_pullback_amd import edit as E
    from diffusion_pullback_amd import main as m
    from oracle import unet_ddpm
    b, a = f["bases"], f["args"]
    cfg = unet_ddpm.DDPMConfig(**b["cfg"])
    params = cf.ddpm_init_params(cfg, seed=b["seed"], spectrum=cf.Spectrum(**b["spectrum"]))
    net = PullbackUNet("ddpm", cfg, params, dtype=torch.float32, device=DEV, max_batch=10, max_rank=16, verbose=False)
    space = {"frechet": "frechet_mean_space", "flag": "flag_mean_space", "hungarian": "hungarian_mean_space"}[job]
    argv = ["--note", "t", "--model_name", a["model_name"], "--dataset_name", a["dataset_name"], "--result_folder", str(tmp), "--device", DEV,
            "--performance_boosting_t", "0.2", "--edit_t", str(a["edit_t"]), "--h_t", str(a["h_t"]), "--seed", str(a["seed"]),
            "--trajectory_batch", str(trajectory_batch), "--edit_ht", "h_space_guidance", "--h_edit_step_size", str(STEP),
            "--no_edit_t", str(round(a["edit_t"] - 0.2, 3)), "--h_guidance_mode", mode, "--local_projection", str(local_projection),
            f"--run_edit_global_{job}_mean_zt", "True", f"--{space}", "h", *extra]
    args = m.preset(m.parse_args(argv))
    args.for_steps = args.inv_steps = a["for_steps"]
    args.image_size = 32
    args.input_root = os.path.join(str(tmp), "inputs")
    ed = E.EditUncondDiffusion(args, unet=net, dataset={0: b["x0"]})
    ed.performance_boosting_t_idx = 1000                   # as in the fixture: the eta = 1 tail draws device noise
    k, n = a["pca_rank"], a["num_local_basis"]
    if job == "frechet":
        basis_path = ed.global_frechet_mean_paths("mid", 0, k, n, "h")[0]
        os.makedirs(os.path.dirname(basis_path), exist_ok=True)
        torch.save(b["global_u"], basis_path)
    else:
        local_dir, local_name = ed._tangent_space_naming("mid", 0, k, dataset_name="Random")
        os.makedirs(local_dir, exist_ok=True)
        for i in range(n):
            torch.save(b["local_u"][i], os.path.join(local_dir, f"u-{local_name(i, a['h_t'])}.pt"))
            torch.save(b["local_vT"][i], os.path.join(local_dir, f"vT-{local_name(i, a['h_t'])}.pt"))
    saved = []
    keep = E.save_image
    E.save_image = lambda x, path, nrow=None: (saved.append((os.path.basename(path), x.detach().float().cpu().clone())), keep(x, path, nrow=nrow))[0]
    kw = dict(op="mid", block_idx=0, vis_num=a["vis_num"], pca_rank=k, num_local_basis=n, local_projection=local_projection, vis_num_pc=a["vis_num_pc"])
    try:
        out = getattr(ed, f"run_edit_global_{job}_mean_zt")(a["idx"], **{space: "h"}, **kw)
    finally:
        E.save_image = keep
    return saved, out, ed


def _records(ed, names):
    return [torch.load(os.path.join(ed.obs_folder, f"hguide-{n}.pt")) for n in names]


@pytest.fixture(scope="module")
def runs(fix, tmp_path_factory):
    return {tb: _run(fix, tmp_path_factory.mktemp(f"hg{tb}"), trajectory_batch=tb) for tb in (1, 20)}


def test_pictures_records_and_the_unedited_row(fix, runs):
    saved, out, ed = runs[20]
    a = fix["args"]
    v = a["vis_num"]
    stem = f"xt-{a['dataset_name']}_{a['idx']}-h_{a['h_t']}T-edit_{a['edit_t']}T-mid-block_0-seed_{a['seed']}-pc_"
    names = [f"{stem}{pc:0=3d}_{tag}" for pc in range(a["vis_num_pc"]) for tag in ("pos", "neg")]
    assert out["names"] == names and out["vk"] is None and len(out["chains"]) == len(names)
    pics = {n: x for n, x in saved if n.startswith("x0_gen-xt-")}
    assert sorted(pics) == sorted(f"x0_gen-{n}.png" for n in names)
    assert all(os.path.exists(os.path.join(ed.result_folder, p)) for p in pics)
    assert sorted(x for x in os.listdir(ed.obs_folder) if x.startswith("hguide-")) == sorted(f"hguide-{n}.pt" for n in names)
    e0, e1 = int(ed.edit_t_idx), int(ed.no_edit_t_idx)
    steps = e1 - e0
    assert steps >= 2
    # the plain DDIM steps over the guided interval, from the job's own x_t
    xT = ed.run_DDIMinversion(idx=a["idx"])
    original = ed.DDIMforwardsteps(xT, t_start_idx=0, t_end_idx=e0)[0]
    plain = ed.DDIMforwardsteps(original, t_start_idx=e0, t_end_idx=e1)[0].cpu()
    recs = dict(zip(names, _records(ed, names)))
    for n, r in recs.items():
        sign = 1.0 if n.endswith("pos") else -1.0
        assert r["mode"] == "asyrp" and r["delta_norm"].shape == (v, steps) and r["dx_norm"].shape == (v, steps) and r["states_end"].shape == (v, 3, 32, 32)
        assert torch.allclose(r["scales"], sign * torch.linspace(0, STEP, v)) and r["timesteps"].tolist() == [float(t) for t in ed.scheduler.timesteps[e0:e1]]
        err = rel(r["states_end"][:1], plain)
        print(n[-10:], "row 0 against the plain steps", err, "dx_norm rows", r["dx_norm"].sum(1).tolist())
        assert err < TOL
        assert (r["dx_norm"][0] == 0).all() and (r["dx_norm"][1:] > 0).all() and (r["delta_norm"][1:] > 0).all()
        # the largest scale moved the latent: two orders of magnitude clear of what separates two routes to the same plain steps (err, or fp32's 2^-24)
        assert rel(r["states_end"][-1:], plain) > 100 * max(err, 2.0 ** -24)
        assert torch.isfinite(pics[f"x0_gen-{n}.png"]).all() and tuple(pics[f"x0_gen-{n}.png"].shape) == (v, 3, 32, 32)
    for pc in range(a["vis_num_pc"]):
        p, q = recs[f"{stem}{pc:0=3d}_pos"], recs[f"{stem}{pc:0=3d}_neg"]
        same = rel(p["states_end"][:1], q["states_end"][:1])                           # both signs start with the unedited row
        assert same < TOL and rel(p["states_end"][1:], q["states_end"][1:]) > 100 * max(same, 2.0 ** -24)


def test_one_experiment_after_another_gives_the_same_files(fix, runs):
    (s1, o1, ed1), (s20, o20, ed20) = runs[1], runs[20]
    assert o1["names"] == o20["names"]
    p1, p20 = {n: x for n, x in s1 if n.startswith("x0_gen-xt-")}, {n: x for n, x in s20 if n.startswith("x0_gen-xt-")}
    assert list(p1) == list(p20)
    for n in p1:
        assert rel(p1[n], p20[n]) < TOL, n
    for a, b in zip(_records(ed1, o1["names"]), _records(ed20, o20["names"])):
        assert rel(a["states_end"], b["states_end"]) < TOL and torch.allclose(a["delta_norm"], b["delta_norm"], rtol=1e-3)


def test_a_second_run_skips_every_experiment_whose_picture_exists(fix, tmp_path):
    saved, out, ed = _run(fix, tmp_path)
    assert len(out["names"]) == 2 * fix["args"]["vis_num_pc"]
    os.remove(os.path.join(ed.result_folder, f"x0_gen-{out['names'][1]}.png"))
    saved2, out2, _ = _run(fix, tmp_path)
    assert out2["names"] == [out["names"][1]] and [n for n, _ in saved2 if n.startswith("x0_gen-xt-")] == [f"x0_gen-{out['names'][1]}.png"]
    saved3, out3, _ = _run(fix, tmp_path)
    assert out3 is None and not [n for n, _ in saved3 if n.startswith("x0_gen-xt-")]       # a finished job does nothing


@pytest.mark.parametrize("job", ["flag", "hungarian"])
def test_the_other_global_basis_jobs_reach_the_same_tail(fix, tmp_path, job):
    saved, out, ed = _run(fix, tmp_path, job=job, mode="symmetric")
    assert len(out["names"]) == 2 * fix["args"]["vis_num_pc"]
    for r in _records(ed, out["names"]):
        assert r["mode"] == "symmetric" and (r["dx_norm"][0] == 0).all() and (r["dx_norm"][1:] > 0).all() and torch.isfinite(r["states_end"]).all()


def test_cli_end_to_end_on_synthetic_weights(tmp_path, monkeypatch):
    """--run_edit_global_frechet_mean_zt True --frechet_mean_space h --edit_ht h_space_guidance --local_projection False --net_scale small: the engine
    sized by main.build_unet, the u- file, the pictures and the records"""
    from diffusion_pullback_amd import main as m
    monkeypatch.chdir(tmp_path)
    preset = m.preset

    def short(args):                                       # 20 DDIM steps instead of the preset's 100: the toy run stays within seconds
        args = preset(args)
        args.for_steps = args.inv_steps = 20
        return args
    monkeypatch.setattr(m, "preset", short)
    argv = ["--note", "t", "--model_name", "CelebA_HQ_HF", "--dataset_name", "Random", "--result_folder", str(tmp_path / "runs"), "--device", DEV,
            "--net_scale", "small", "--performance_boosting_t", "0.2", "--edit_t", "0.8", "--h_t", "0.8", "--run_edit_global_frechet_mean_zt", "True",
            "--frechet_mean_space", "h", "--num_local_basis", "4", "--pca_rank", "3", "--vis_num_pc", "2", "--vis_num", "3", "--frechet_max_iter", "200",
            "--edit_ht", "h_space_guidance", "--h_edit_step_size", "8", "--no_edit_t", "0.5", "--local_projection", "False"]
    ed = m.main(argv)
    assert ed.edit_ht == "h_space_guidance" and ed.edit_xt == "parallel-x" and ed.unet.engine.max_batch >= 2
    stem = "xt-Random_0-h_0.8T-edit_0.8T-mid-block_0-seed_0-pc_00"
    names = [stem + s for s in ("0_neg", "0_pos", "1_neg", "1_pos")]
    assert sorted(x for x in os.listdir(ed.result_folder) if x.startswith("x0_gen-")) == [f"x0_gen-{n}.png" for n in names]
    assert sorted(x for x in os.listdir(ed.obs_folder) if x.startswith("hguide-")) == [f"hguide-{n}.pt" for n in names]
    for rec in _records(ed, names):
        steps = int(ed.no_edit_t_idx) - int(ed.edit_t_idx)
        assert rec["delta_norm"].shape == (3, steps) and (rec["dx_norm"][0] == 0).all() and (rec["dx_norm"][1:] > 0).all()
