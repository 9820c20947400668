"""EditUncondDiffusion.run_edit_global_frechet_mean_zt on the HIP engine against the run recorded from the reference's own method on the vendored
PullBackDDPM (tests/golden/make_golden_frechet.py), spaces x and h with local_projection: the vk of every chain, every U-Net input on the sequential
path and the pictures at the bars of tests/test_gpu_transport_job.py (relative error < 2e-3); the global basis computed here from the four pre-placed
local bases within 1e-6 rad of the fixture's (tests/_frechet_ref.py); the skip rule; chains together against one at a time; the CLI end to end."""
import os

import numpy as np
import pytest
import torch

import _frechet_ref as R
from _util import load_golden, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-3


class _Rec:
    """records every U-Net call (t, input) and every local_encoder_pullback_batch call of a driver run; everything else is the wrapped PullbackUNet's"""

    def __init__(self, net):
        self._net, self.calls, self.pullbacks = net, [], []

    def __call__(self, x, t, *a, **k):
        self.calls.append((float(t), x.detach().float().cpu().clone()))
        return self._net(x, t, *a, **k)

    def local_encoder_pullback_batch(self, samples, timesteps, *a, **k):
        self.pullbacks.append((int(samples.shape[0]), [float(t) for t in timesteps]))
        return self._net.local_encoder_pullback_batch(samples, timesteps, *a, **k)

    def __getattr__(self, n):
        return getattr(self._net, n)


@pytest.fixture(scope="module")
def fix():
    f = load_golden("frechet_uncond_small.pt")
    rows = torch.cat([load_golden(n) for n in f["trace_files"]])
    saved = load_golden("frechet_uncond_small.saved.pt")
    r0 = 0
    for space in ("x", "h"):
        run = f["runs"][space]
        n = sum(run["trace_batch"])
        run["trace_x"] = list(rows[r0:r0 + n].split(run["trace_batch"]))
        run["saved"] = saved[space]
        r0 += n
    assert r0 == rows.shape[0]
    return f


def _run(f, tmp, space, trajectory_batch, max_batch, place_global):
    """one run of the job on the fixture's toy net with the four local bases and the sample's own in place; place_global: the fixture's global basis
    too (the load branch, as the reference ran).  Returns the recorder, the save_image calls, the job's return value and the driver."""
    from diffusion_pullback_amd import PullbackUNet, configs as cf
    from diffusion_pullback_amd import edit as E
    from diffusion_pullback_amd import main as m
    from oracle import unet_ddpm
    a = f["args"]
    cfg = unet_ddpm.DDPMConfig(**f["cfg"])
    params = cf.ddpm_init_params(cfg, seed=f["seed"], spectrum=cf.Spectrum(**f["spectrum"]))
    net = _Rec(PullbackUNet("ddpm", cfg, params, dtype=torch.float32, device=DEV, max_batch=max_batch, max_rank=4, verbose=False))
    argv = ["--note", "t", "--model_name", a["model_name"], "--dataset_name", a["dataset_name"], "--result_folder", str(tmp), "--device", DEV,
            "--performance_boosting_t", "0.2", "--x_space_guidance_edit_step", str(a["x_space_guidance_edit_step"]), "--x_space_guidance_scale",
            str(a["x_space_guidance_scale"]), "--x_space_guidance_num_step", str(a["x_space_guidance_num_step"]), "--edit_t", str(a["edit_t"]),
            "--h_t", str(a["h_t"]), "--seed", str(a["seed"]), "--trajectory_batch", str(trajectory_batch)]
    args = m.preset(m.parse_args(argv))
    args.for_steps = args.inv_steps = a["for_steps"]
    args.image_size = 32
    args.input_root = os.path.join(str(tmp), "inputs")
    ed = E.EditUncondDiffusion(args, unet=net, dataset={0: f["x0"]})
    ed.performance_boosting_t_idx = 1000                   # as in the fixture: the eta = 1 tail draws device noise
    assert int(ed.edit_t_idx) == f["edit_t_idx"]
    k, n = a["pca_rank"], a["num_local_basis"]
    local_dir, local_name = ed._tangent_space_naming("mid", 0, k, dataset_name="Random")
    own_dir, own_name = ed._tangent_space_naming("mid", 0, k)
    os.makedirs(local_dir, exist_ok=True); os.makedirs(own_dir, exist_ok=True)
    for i in range(n):
        torch.save(f["local_u"][i], os.path.join(local_dir, f"u-{local_name(i, a['h_t'])}.pt"))
        torch.save(f["local_vT"][i], os.path.join(local_dir, f"vT-{local_name(i, a['h_t'])}.pt"))
    torch.save(f["own_u"], os.path.join(own_dir, f"u-{own_name(0, a['h_t'])}.pt"))
    torch.save(f["own_vT"], os.path.join(own_dir, f"vT-{own_name(0, a['h_t'])}.pt"))
    basis_path, info_path = ed.global_frechet_mean_paths("mid", 0, k, n, space)
    if place_global:
        os.makedirs(os.path.dirname(basis_path), exist_ok=True)
        torch.save(f["global_v" if space == "x" else "global_u"], basis_path)
    saved = []
    keep = E.save_image
    E.save_image = lambda x, path, nrow=None: saved.append((os.path.basename(path), x.detach().float().cpu().clone()))
    try:
        torch.manual_seed(a["rng_seed"])
        out = ed.run_edit_global_frechet_mean_zt(a["idx"], op="mid", block_idx=0, vis_num=a["vis_num"], pca_rank=k, num_local_basis=n,
                                                 local_projection=True, frechet_mean_space=space, frechet_tol=1e-10, **a["runs"][space])
    finally:
        E.save_image = keep
    return net, saved, out, ed, (basis_path, info_path)


@pytest.fixture(scope="module")
def sequential(fix, tmp_path_factory):
    return {s: _run(fix, tmp_path_factory.mktemp("seq" + s), s, trajectory_batch=1, max_batch=5, place_global=True) for s in ("x", "h")}


@pytest.fixture(scope="module")
def computed(fix, tmp_path_factory):
    return {s: _run(fix, tmp_path_factory.mktemp("own" + s), s, trajectory_batch=20, max_batch=20, place_global=False) for s in ("x", "h")}


@pytest.mark.parametrize("space", ["x", "h"])
def test_sequential_path_matches_the_reference_call_by_call(fix, sequential, space):
    """the fixture's global basis in place (the reference's load branch), trajectory_batch = 1: the vk of both chains, all 64 U-Net inputs (18 inversion
    steps, 8 to edit_t, per chain 8 guidance calls of batch 2 and 11 decode calls of batch 5) and every picture, names and order included"""
    net, saved, out, ed, _ = sequential[space]
    r = fix["runs"][space]
    assert out["names"] == r["names"] and out["info"] is None and net.pullbacks == []
    for sign, want in zip((1, -1), r["vk"]):
        err = rel(sign * out["vk"][0].cpu(), want)
        print(f"space {space}: vk ({'+' if sign > 0 else '-'}) relative error {err:.2e}")
        assert err < TOL
    assert len(net.calls) == len(r["trace_t"]) == 64
    worst = 0.0
    for i, (t, x) in enumerate(net.calls):
        assert t == r["trace_t"][i], (i, t, r["trace_t"][i])
        assert x.shape == r["trace_x"][i].shape, (i, x.shape, r["trace_x"][i].shape)
        worst = max(worst, rel(x, r["trace_x"][i]))
    print(f"space {space}: worst relative U-Net input error {worst:.2e}")
    assert worst < TOL
    assert [n for n, _ in saved] == [n for n, _ in r["saved"]]
    errs = {n: rel(x, w) for (n, x), (_, w) in zip(saved, r["saved"])}
    print("pictures:", {n[-22:]: f"{e:.2e}" for n, e in errs.items()})
    assert max(errs.values()) < TOL
    if os.path.isdir(ed.obs_folder) and os.listdir(ed.obs_folder):          # (written only where matplotlib is installed)
        assert sorted(os.listdir(ed.obs_folder)) == sorted(r["plots"])


@pytest.mark.parametrize("space", ["x", "h"])
def test_the_job_computes_the_basis_the_restatement_computes(fix, sequential, computed, space):
    """no global-basis file: the mean of the four pre-placed local bases on the GPU, written as [N, k] columns with an info file; its span within 1e-6 rad
    of the fixture's, the pictures those of the run on the fixture's basis, chains together (the default) against one at a time"""
    net, saved, out, ed, (basis_path, info_path) = computed[space]
    want = fix["global_v" if space == "x" else "global_u"]
    cols = torch.load(basis_path)
    assert tuple(cols.shape) == tuple(want.shape) and cols.dtype == torch.float32
    ang = R.max_angle(cols.numpy().T, want.numpy().T)
    ref = fix["global_info"][space]
    info = torch.load(info_path, weights_only=False)
    print(f"space {space}: computed basis against the fixture's {ang:.2e} rad; {info['iterations']} steps (restatement {ref['iterations']}), "
          f"weight error {np.abs(info['weight'].numpy() - ref['weight']).max():.2e}")
    assert ang <= 1e-6
    assert info["converged"] and info["space"] == space and len(info["names"]) == 4 and len(info["cost"]) == info["iterations"] + 1
    assert np.abs(info["weight"].numpy() - ref["weight"]).max() <= 1e-6 and np.abs(info["theta"].numpy() - ref["theta"]).max() <= 1e-6
    assert net.pullbacks == []
    n_pre = 26
    assert [c[1].shape[0] for c in net.calls[:n_pre]] == [1] * n_pre
    assert [c[1].shape[0] for c in net.calls[n_pre:]] == [4] * 8 + [10] * 11            # 2 chains: 4 rows per guidance step, 10 decode states
    # row signs of a computed basis are the solver's: the +- pair is the same two directions, possibly under each other's names
    vk, vk_seq = out["vk"][0].cpu(), sequential[space][2]["vk"][0].cpu()
    flipped = rel(vk, vk_seq) > rel(-vk, vk_seq)
    assert min(rel(vk, vk_seq), rel(-vk, vk_seq)) < TOL
    swap = lambda n: n.replace("_pos.", "_tmp.").replace("_neg.", "_pos.").replace("_tmp.", "_neg.") if flipped else n
    seq = {swap(n): x for n, x in sequential[space][1]}
    errs = {n: rel(x, seq[n]) for n, x in saved}
    print(f"space {space}: together on the computed basis vs one at a time on the fixture's (row sign flipped: {flipped}): {max(errs.values()):.2e}")
    assert sorted(n for n, _ in saved) == sorted(seq) and max(errs.values()) < TOL


def test_a_finished_job_does_nothing(fix, computed):
    net, saved, _, ed, _ = computed["x"]
    calls = len(net.calls)
    for n, _ in saved:                                        # save_image was captured: put the pictures where the job looks for them
        if n.startswith("x0_gen-"):
            open(os.path.join(ed.result_folder, n), "w").close()
    a = fix["args"]
    assert ed.run_edit_global_frechet_mean_zt(a["idx"], vis_num=a["vis_num"], pca_rank=a["pca_rank"], num_local_basis=a["num_local_basis"],
                                              frechet_mean_space="x", **a["runs"]["x"]) is None
    assert len(net.calls) == calls


def test_cli_end_to_end_on_synthetic_weights(tmp_path, monkeypatch):
    """--run_edit_global_frechet_mean_zt True --frechet_mean_space x --num_local_basis 8 --net_scale small: the engine sized by main.build_unet, the
    eight local bases sampled in groups, the v- file, the info file and the pictures"""
    from diffusion_pullback_amd import main as m
    monkeypatch.chdir(tmp_path)
    preset = m.preset

    def short(args):                                       # 20 DDIM steps instead of the preset's 100: the toy run stays within seconds
        args = preset(args)
        args.for_steps = args.inv_steps = 20
        return args
    monkeypatch.setattr(m, "preset", short)
    argv = ["--note", "t", "--model_name", "CelebA_HQ_HF", "--dataset_name", "Random", "--result_folder", str(tmp_path / "runs"), "--device", DEV,
            "--net_scale", "small", "--performance_boosting_t", "0.2", "--x_space_guidance_scale", "0.1", "--x_space_guidance_num_step", "4",
            "--edit_t", "0.6", "--h_t", "0.8", "--run_edit_global_frechet_mean_zt", "True", "--frechet_mean_space", "x", "--num_local_basis", "8",
            "--pca_rank", "3", "--vis_num_pc", "1", "--frechet_max_iter", "200"]
    ed = m.main(argv)
    assert ed.unet.engine.max_batch >= 8 and ed.unet.max_rank >= 24
    basis_path, info_path = ed.global_frechet_mean_paths("mid", 0, 3, 8, "x")
    assert basis_path.startswith(os.path.join("./inputs", "global_frechet_mean_uncond-model_CelebA_HQ_HF-dataset_Random-num_steps_20-pca_rank_3"))
    assert os.path.basename(basis_path) == "v-0.8T-mid-block_0-seed_0-num_local_basis_8.pt"
    cols, info = torch.load(basis_path), torch.load(info_path, weights_only=False)
    assert tuple(cols.shape) == (3 * 32 * 32, 3) and torch.isfinite(cols).all()
    assert torch.allclose(cols.t() @ cols, torch.eye(3), atol=1e-5)
    assert (np.diff(info["cost"]) <= 1e-12 * info["cost"][:-1] + 1e-14).all() and len(info["names"]) == 8
    local = os.path.join("./inputs", "local_encoder_pullback_uncond-model_CelebA_HQ_HF-dataset_Random-num_steps_20-pca_rank_3")
    assert len([x for x in os.listdir(local) if x.startswith("vT-xt-Random_")]) == 8
    res = os.listdir(ed.result_folder)
    stem = "x0_gen-xt-Random_0-h_0.8T-edit_0.6T-mid-block_0-seed_0-pc_000_"
    assert sorted(x for x in res if x.startswith("x0_gen-")) == [stem + "neg.png", stem + "pos.png"]
