"""EditUncondDiffusion.run_edit_global_hungarian_mean_zt on the HIP engine against the run recorded from the reference's own method on the vendored
PullBackDDPM (tests/golden/make_golden_hungarian.py; net, sample and local bases are those of the Frechet fixture): the vk of every chain, every U-Net
input on the sequential path and the pictures at the bars of tests/test_gpu_frechet_job.py (relative error < 2e-3); the two global bases computed here
from the four pre-placed local bases against the restatement's (tests/_hungarian_ref.py: perm and sign exact, every element within
2^-23 |Y_ref| + 1e-12); space h against its definition; the skip rule; chains together against one at a time; the info- mismatch error; the CLI end to
end."""
import os
import re

import numpy as np
import pytest
import torch

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
    f = load_golden("hungarian_uncond_small.pt")
    f["base"] = load_golden(f["base"])
    rows = torch.cat([load_golden(n) for n in f["trace_files"]])
    assert rows.shape[0] == sum(f["run"]["trace_batch"])
    f["run"]["trace_x"] = list(rows.split(f["run"]["trace_batch"]))
    f["run"]["saved"] = load_golden("hungarian_uncond_small.saved.pt")
    return f


def _run(f, tmp, space, trajectory_batch, max_batch, place_global, **kw):
    """one run of the job on the fixture's toy net with the four local bases and the sample's own in place; place_global: the fixture's two global
    bases too (the load branch, as the reference ran).  Returns the recorder, the save_image calls, the job's return value, the driver, the paths."""
    from diffusion_pullback_amd import PullbackUNet, configs as cf
    from diffusion_pullback_amd import edit as E
    from diffusion_pullback_amd import main as m
    from oracle import unet_ddpm
    a, g = f["args"], f["base"]
    cfg = unet_ddpm.DDPMConfig(**g["cfg"])
    params = cf.ddpm_init_params(cfg, seed=g["seed"], spectrum=cf.Spectrum(**g["spectrum"]))
    net = _Rec(PullbackUNet("ddpm", cfg, params, dtype=torch.float32, device=DEV, max_batch=max_batch, max_rank=4, verbose=False))
    argv = ["--note", "t", "--model_name", a["model_name"], "--dataset_name", a["dataset_name"], "--result_folder", str(tmp), "--device", DEV,
            "--performance_boosting_t", "0.2", "--x_space_guidance_edit_step", str(a["x_space_guidance_edit_step"]), "--x_space_guidance_scale",
            str(a["x_space_guidance_scale"]), "--x_space_guidance_num_step", str(a["x_space_guidance_num_step"]), "--edit_t", str(a["edit_t"]),
            "--h_t", str(a["h_t"]), "--seed", str(a["seed"]), "--trajectory_batch", str(trajectory_batch)]
    args = m.preset(m.parse_args(argv))
    args.for_steps = args.inv_steps = a["for_steps"]
    args.image_size = 32
    args.input_root = os.path.join(str(tmp), "inputs")
    ed = E.EditUncondDiffusion(args, unet=net, dataset={0: g["x0"]})
    ed.performance_boosting_t_idx = 1000                   # as in the fixture: the eta = 1 tail draws device noise
    assert int(ed.edit_t_idx) == g["edit_t_idx"]
    k, n = a["pca_rank"], a["num_local_basis"]
    local_dir, local_name = ed._tangent_space_naming("mid", 0, k, dataset_name="Random")
    own_dir, own_name = ed._tangent_space_naming("mid", 0, k)
    os.makedirs(local_dir, exist_ok=True); os.makedirs(own_dir, exist_ok=True)
    for i in range(n):
        torch.save(g["local_u"][i], os.path.join(local_dir, f"u-{local_name(i, a['h_t'])}.pt"))
        torch.save(g["local_vT"][i], os.path.join(local_dir, f"vT-{local_name(i, a['h_t'])}.pt"))
    torch.save(g["own_u"], os.path.join(own_dir, f"u-{own_name(0, a['h_t'])}.pt"))
    torch.save(g["own_vT"], os.path.join(own_dir, f"vT-{own_name(0, a['h_t'])}.pt"))
    paths = ed.global_hungarian_mean_paths("mid", 0, k)
    if place_global:
        os.makedirs(os.path.dirname(paths["u"][0]), exist_ok=True)
        torch.save(f["global_u"], paths["u"][0])
        torch.save(f["global_v"], paths["v"][0])
    saved = []
    keep = E.save_image
    E.save_image = lambda x, path, nrow=None: saved.append((os.path.basename(path), x.detach().float().cpu().clone()))
    try:
        torch.manual_seed(a["rng_seed"])
        out = ed.run_edit_global_hungarian_mean_zt(a["idx"], op="mid", block_idx=0, vis_num=a["vis_num"], pca_rank=k, num_local_basis=n,
                                                   local_projection=True, hungarian_mean_space=space, **dict(a["run"], **kw))
    finally:
        E.save_image = keep
    return net, saved, out, ed, paths


@pytest.fixture(scope="module")
def sequential(fix, tmp_path_factory):
    return _run(fix, tmp_path_factory.mktemp("seq"), "x", trajectory_batch=1, max_batch=5, place_global=True)


@pytest.fixture(scope="module")
def computed(fix, tmp_path_factory):
    return _run(fix, tmp_path_factory.mktemp("own"), "x", trajectory_batch=20, max_batch=20, place_global=False)


def test_sequential_path_matches_the_reference_call_by_call(fix, sequential):
    """both global bases in place (the reference's load branch), trajectory_batch = 1: the vk of both chains, all 64 U-Net inputs (18 inversion steps, 8
    to edit_t, per chain 8 guidance calls of batch 2 and 11 decode calls of batch 5) and every picture, names and order included"""
    net, saved, out, ed, _ = sequential
    r = fix["run"]
    assert out["names"] == r["names"] and out["info"] is None and net.pullbacks == []
    for sign, want in zip((1, -1), r["vk"]):
        err = rel(sign * out["vk"][0].cpu(), want)
        print(f"vk ({'+' if sign > 0 else '-'}) relative error {err:.2e}")
        assert err < TOL
    assert len(net.calls) == len(r["trace_t"]) == 64
    worst = 0.0
    for i, (t, x) in enumerate(net.calls):
        assert t == r["trace_t"][i], (i, t, r["trace_t"][i])
        assert x.shape == r["trace_x"][i].shape, (i, x.shape, r["trace_x"][i].shape)
        worst = max(worst, rel(x, r["trace_x"][i]))
    print(f"worst relative U-Net input error {worst:.2e}")
    assert worst < TOL
    assert [n for n, _ in saved] == [n for n, _ in r["saved"]]
    errs = {n: rel(x, w) for (n, x), (_, w) in zip(saved, r["saved"])}
    print("pictures:", {n[-22:]: f"{e:.2e}" for n, e in errs.items()})
    assert max(errs.values()) < TOL
    if os.path.isdir(ed.obs_folder) and os.listdir(ed.obs_folder):          # (written only where matplotlib is installed)
        assert sorted(os.listdir(ed.obs_folder)) == sorted(r["plots"])


def test_chains_together_match_one_at_a_time(fix, sequential, tmp_path):
    net, saved, out, _, _ = _run(fix, tmp_path, "x", trajectory_batch=20, max_batch=20, place_global=True)
    n_pre = 26
    assert [c[1].shape[0] for c in net.calls[:n_pre]] == [1] * n_pre
    assert [c[1].shape[0] for c in net.calls[n_pre:]] == [4] * 8 + [10] * 11            # 2 chains: 4 rows per guidance step, 10 decode states
    assert torch.equal(out["vk"], sequential[2]["vk"])
    seq = dict(sequential[1])
    errs = {n: rel(x, seq[n]) for n, x in saved}
    print(f"together vs one at a time: {max(errs.values()):.2e}")
    assert sorted(n for n, _ in saved) == sorted(seq) and max(errs.values()) < TOL


def test_the_job_computes_the_bases_the_restatement_computes(fix, computed):
    """no global-basis file: both matched means of the four pre-placed local bases on the GPU, written as [N, k] columns with an info file each"""
    net, saved, out, ed, paths = computed
    assert net.pullbacks == []
    for tag in ("u", "v"):
        want, ref = fix["global_" + tag], fix["global_info"][tag]
        cols, info = torch.load(paths[tag][0]), torch.load(paths[tag][1], weights_only=False)
        assert tuple(cols.shape) == tuple(want.shape) and cols.dtype == torch.float32
        err = (cols.double() - want.double()).abs()
        bar = 2.0 ** -23 * want.double().abs() + 1e-12
        print(f"{tag}: computed basis against the restatement's: worst error {float((err / bar).max()):.3f} of the bar; {info['sweeps']} sweeps, "
              f"weight error {np.abs(info['weight'].numpy() - ref['weight']).max():.2e}")
        assert (info["perm"].numpy() == ref["perm"]).all() and (info["sign"].numpy() == ref["sign"]).all()
        assert bool((err <= bar).all())
        assert info["converged"] and info["sweeps"] == ref["sweeps"] and info["changed"] == ref["changed"]
        assert info["num_local_basis"] == 4 and info["distance"] == "1/cosine" and len(info["names"]) == 4
        assert np.abs(info["cost"] - ref["cost"]).max() <= 1e-9 * np.abs(ref["cost"]).max()
        assert np.abs(info["weight"].numpy() - ref["weight"]).max() <= 2.0 ** -23
        assert torch.equal(out["basis_" + tag].cpu(), cols.t())
    assert set(out["info"]) == {"u", "v"} and len(out["names"]) == 2 and torch.isfinite(out["vk"]).all()


def test_space_h_follows_its_definition(fix, tmp_path):
    """vk = normalise(vT^T (u^T uhat_pc)) with the sample's own unit (u, vT) and the global u basis, in float64"""
    net, saved, out, ed, _ = _run(fix, tmp_path, "h", trajectory_batch=20, max_batch=20, place_global=True)
    g = fix["base"]
    u, vT = g["own_u"].double(), g["own_vT"].double()
    u, vT = u / u.norm(dim=0, keepdim=True), vT / vT.norm(dim=1, keepdim=True)
    gu = fix["global_u"].double()
    uk = gu[:, 1] / gu[:, 1].norm()
    want = vT.t() @ (u.t() @ uk)
    want = want / want.norm()
    err = rel(out["vk"][0].cpu(), want)
    print(f"space h: vk against its float64 definition {err:.2e}")
    assert err < 1e-5                                        # (the fp32 stream of dpb_transport_directions: its own tests hold it to 1e-5)
    assert len(saved) and all(torch.isfinite(x).all() for _, x in saved)
    with pytest.raises(ValueError, match="local_projection"):
        ed.run_edit_global_hungarian_mean_zt(0, vis_num_pc=1, pca_rank=4, num_local_basis=4, hungarian_mean_space="h", local_projection=False)
    with pytest.raises(ValueError, match="hungarian_mean_space"):
        ed.run_edit_global_hungarian_mean_zt(0, vis_num_pc=1, pca_rank=4, num_local_basis=4, hungarian_mean_space="z")


def test_a_finished_job_does_nothing_and_a_mismatched_info_file_raises(fix, computed):
    net, saved, _, ed, paths = computed
    a = fix["args"]
    kw = dict(vis_num=a["vis_num"], pca_rank=a["pca_rank"], **a["run"])
    with pytest.raises(ValueError, match=re.escape(os.path.basename(paths["u"][1]))):                  # the cached bases are those of 4 local bases
        ed.run_edit_global_hungarian_mean_zt(a["idx"], num_local_basis=3, **kw)
    with pytest.raises(ValueError, match="info-"):
        ed.run_edit_global_hungarian_mean_zt(a["idx"], num_local_basis=4, hungarian_distance="cosine", **kw)
    calls = len(net.calls)
    for n, _ in saved:                                        # save_image was captured: put the pictures where the job looks for them
        if n.startswith("x0_gen-"):
            open(os.path.join(ed.result_folder, n), "w").close()
    assert ed.run_edit_global_hungarian_mean_zt(a["idx"], num_local_basis=a["num_local_basis"], **kw) is None
    assert len(net.calls) == calls


def test_cli_end_to_end_on_synthetic_weights(tmp_path, monkeypatch):
    """--run_edit_global_hungarian_mean_zt True --num_local_basis 8 --net_scale small: the engine sized by main.build_unet, the eight local bases
    sampled in groups, the u- / v- files, their info files and the pictures"""
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
            "--edit_t", "0.6", "--h_t", "0.8", "--run_edit_global_hungarian_mean_zt", "True", "--hungarian_mean_space", "x", "--num_local_basis", "8",
            "--pca_rank", "3", "--vis_num_pc", "1"]
    ed = m.main(argv)
    assert ed.unet.engine.max_batch >= 8 and ed.unet.max_rank >= 24
    paths = ed.global_hungarian_mean_paths("mid", 0, 3)
    assert paths["v"][0].startswith(os.path.join("./inputs", "global_hungarian_mean_uncond-model_CelebA_HQ_HF-dataset_Random-num_steps_20-pca_rank_3"))
    assert os.path.basename(paths["v"][0]) == "v-0.8T-mid-block_0-seed_0.pt" and os.path.basename(paths["u"][1]) == "info-u-0.8T-mid-block_0-seed_0.pt"
    for tag, n in (("u", None), ("v", 3 * 32 * 32)):
        cols, info = torch.load(paths[tag][0]), torch.load(paths[tag][1], weights_only=False)
        assert cols.shape[1] == 3 and (n is None or cols.shape[0] == n) and torch.isfinite(cols).all()
        assert torch.allclose(cols.norm(dim=0), torch.ones(3), atol=1e-6)
        assert tuple(info["perm"].shape) == (8, 3) and (info["perm"].sort(dim=1).values == torch.arange(3)).all()
        assert info["sign"].abs().eq(1).all() and info["sweeps"] == len(info["changed"]) <= 20
        assert info["num_local_basis"] == 8 and info["distance"] == "1/cosine" and len(info["names"]) == 8 and info["cost"].shape[1] == 8
    local = os.path.join("./inputs", "local_encoder_pullback_uncond-model_CelebA_HQ_HF-dataset_Random-num_steps_20-pca_rank_3")
    assert len([x for x in os.listdir(local) if x.startswith("vT-xt-Random_")]) == 8
    res = os.listdir(ed.result_folder)
    stem = "x0_gen-xt-Random_0-h_0.8T-edit_0.6T-mid-block_0-seed_0-pc_000_"
    assert sorted(x for x in res if x.startswith("x0_gen-")) == [stem + "neg.png", stem + "pos.png"]
