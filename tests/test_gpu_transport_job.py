"""EditUncondDiffusion.run_edit_parallel_transport on the HIP engine against the run recorded from the reference's own method on the vendored
PullBackDDPM (tests/golden/make_golden_transport.py): the pictures and, on the sequential path, every U-Net input at the bar of
test_uncond_driver_matches_reference_driver_fixture (relative error < 2e-3); chains together against one at a time at the bar
_edit_trajectories_together documents (< 2e-3 on fp32 engines); bases computed from scratch in one batched call; a list of targets; the ADM kind."""
import os

import pytest
import torch

from _util import abs_cos, load_golden, rel

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
    f = load_golden("transport_uncond_small.pt")
    rows = torch.cat([load_golden(n) for n in f["trace_files"]])
    assert rows.shape[0] == sum(f["trace_batch"])
    f["trace_x"] = list(rows.split(f["trace_batch"]))
    return f


def _run(f, tmp, trajectory_batch, max_batch, max_rank, place=(0, 1), targets=1, vis_num_pc=None, extra=None):
    """one run of the job on the fixture's toy net; place: the samples whose fixture bases are put where the job looks for them.  Returns the recorder,
    the save_image calls, the job's return value, the driver and the basis directory."""
    from diffusion_pullback_amd import PullbackUNet, configs as cf
    from diffusion_pullback_amd import edit as E
    from diffusion_pullback_amd import geometry
    from diffusion_pullback_amd import main as m
    from oracle import unet_ddpm
    a = f["args"]
    cfg = unet_ddpm.DDPMConfig(**f["cfg"])
    params = cf.ddpm_init_params(cfg, seed=f["seed"], spectrum=cf.Spectrum(**f["spectrum"]))
    net = _Rec(PullbackUNet("ddpm", cfg, params, dtype=torch.float32, device=DEV, max_batch=max_batch, max_rank=max_rank, verbose=False))
    argv = ["--note", "t", "--model_name", a["model_name"], "--dataset_name", a["dataset_name"], "--result_folder", str(tmp), "--device", DEV,
            "--performance_boosting_t", "0.2", "--x_space_guidance_edit_step", str(a["x_space_guidance_edit_step"]), "--x_space_guidance_scale",
            str(a["x_space_guidance_scale"]), "--x_space_guidance_num_step", str(a["x_space_guidance_num_step"]), "--edit_t", str(a["edit_t"]),
            "--h_t", str(a["h_t"]), "--seed", str(a["seed"]), "--trajectory_batch", str(trajectory_batch)]
    args = m.preset(m.parse_args(argv))
    args.for_steps = args.inv_steps = a["for_steps"]
    args.image_size = 32
    args.input_root = os.path.join(str(tmp), "inputs")
    dataset = {0: f["x0"][0], 1: f["x0"][1]}
    dataset.update(extra or {})
    ed = E.EditUncondDiffusion(args, unet=net, dataset=dataset)
    ed.performance_boosting_t_idx = 1000                   # as in the fixture: the eta = 1 tail draws device noise
    assert int(ed.edit_t_idx) == f["edit_t_idx"]
    save_dir, exp_name = ed._tangent_space_naming("mid", 0, a["pca_rank"])
    os.makedirs(save_dir, exist_ok=True)
    for i in place:
        torch.save(f["u"][i], os.path.join(save_dir, f"u-{exp_name(i, a['h_t'])}.pt"))
        torch.save(f["vT"][i], os.path.join(save_dir, f"vT-{exp_name(i, a['h_t'])}.pt"))
    saved, transports = [], []
    keep, keep_t = E.save_image, geometry.transport_directions

    def counted(u_src, u_dst, *a_, **k_):
        transports.append(tuple(u_dst.shape))
        return keep_t(u_src, u_dst, *a_, **k_)
    E.save_image = lambda x, path, nrow=None: saved.append((os.path.basename(path), x.detach().float().cpu().clone()))
    geometry.transport_directions = counted
    try:
        torch.manual_seed(a["rng_seed"])
        out = ed.run_edit_parallel_transport(a["sample_idx_0"], targets, op="mid", block_idx=0, vis_num=a["vis_num"],
                                             vis_num_pc=a["vis_num_pc"] if vis_num_pc is None else vis_num_pc, pca_rank=a["pca_rank"])
    finally:
        E.save_image, geometry.transport_directions = keep, keep_t
    net.transports = transports
    return net, saved, out, ed, save_dir


@pytest.fixture(scope="module")
def sequential(fix, tmp_path_factory):
    return _run(fix, tmp_path_factory.mktemp("seq"), trajectory_batch=1, max_batch=5, max_rank=4)


@pytest.fixture(scope="module")
def together(fix, tmp_path_factory):
    return _run(fix, tmp_path_factory.mktemp("tog"), trajectory_batch=20, max_batch=20, max_rank=4)


def _pictures(saved):
    return [(n, x) for n, x in saved if n.startswith(("x0_gen-", "vk-"))]


def test_sequential_path_matches_the_reference_call_by_call(fix, sequential):
    """trajectory_batch = 1 with the fixture's bases in place: all 212 U-Net inputs (2 x 18 inversion steps, 2 x 4 steps to h_t, 2 x 8 to edit_t, then per
    chain 8 guidance calls of batch 2 and 11 decode calls of batch 5) and every picture, names and order included"""
    net, saved, out, ed, _ = sequential
    f = fix
    assert len(net.calls) == len(f["trace_t"]) == 212 and net.pullbacks == []
    worst = 0.0
    for i, (t, x) in enumerate(net.calls):
        assert t == f["trace_t"][i], (i, t, f["trace_t"][i])
        assert x.shape == f["trace_x"][i].shape, (i, x.shape, f["trace_x"][i].shape)
        worst = max(worst, rel(x, f["trace_x"][i]))
    print("sequential path: worst relative U-Net input error", worst)
    assert worst < TOL
    assert [n for n, _ in saved] == [n for n, _ in f["saved"]]
    errs = {n: rel(x, r) for (n, x), (_, r) in zip(saved, f["saved"])}
    print("pictures:", {n[-22:]: f"{e:.2e}" for n, e in errs.items()})
    assert max(errs.values()) < TOL
    assert out["names"] == [n[len("x0_gen-"):-len(".png")] for n, _ in f["saved"] if n.startswith("x0_gen-xt-")]
    assert float(out["coef_norm"].max()) <= 1 + 1e-6


def test_chains_together_match_one_at_a_time(fix, sequential, together):
    """the default: the 8 chains in ONE U-Net call of 16 rows per guidance step and the 40 decode states in calls of the engine's batch; same files"""
    net, saved, out, _, _ = together
    n_pre = 60
    assert [c[1].shape[0] for c in net.calls[:n_pre]] == [1] * n_pre
    assert [c[1].shape[0] for c in net.calls[n_pre:]] == [16] * 8 + [20, 20] * 11
    assert net.transports == [(1, 4, fix["u"][0].shape[0])]
    seq = dict(_pictures(sequential[1]))
    got = _pictures(saved)
    assert sorted(n for n, _ in got) == sorted(seq)
    errs = {n: rel(x, seq[n]) for n, x in got}
    print("together vs one at a time:", max(errs.values()))
    assert max(errs.values()) < TOL
    ref = dict(fix["saved"])
    assert max(rel(x, ref[n]) for n, x in got) < TOL           # and against the reference's own pictures
    for a, b in zip(out["vk"], sequential[2]["vk"]):           # the directions do not depend on how the chains are batched
        assert torch.equal(a, b)


def test_a_finished_job_does_nothing(fix, together):
    net, saved, _, ed, _ = together
    from diffusion_pullback_amd import edit as E
    calls = len(net.calls)
    for n, _ in saved:                                        # save_image was captured: put the pictures where the job looks for them
        if n.startswith("x0_gen-"):
            open(os.path.join(ed.result_folder, n), "w").close()
    a = fix["args"]
    assert ed.run_edit_parallel_transport(a["sample_idx_0"], a["sample_idx_1"], vis_num=a["vis_num"], vis_num_pc=a["vis_num_pc"], pca_rank=a["pca_rank"]) is None
    assert len(net.calls) == calls


def test_bases_from_scratch_come_from_one_batched_pullback(fix, tmp_path):
    """no basis files: both bases from ONE local_encoder_pullback_batch call of two samples at t(h_t), saved as u- / s- / vT-; the leading transported
    direction agrees with the reference's up to sign at |cos| >= 0.99 (the README's 16-bit parity bar: the fixture's bases stopped at the
    reference's own iteration count)"""
    f, a = fix, fix["args"]
    net, saved, out, ed, save_dir = _run(f, tmp_path, trajectory_batch=20, max_batch=20, max_rank=8, place=())
    assert len(net.pullbacks) == 1 and net.pullbacks[0][0] == 2 and len(set(net.pullbacks[0][1])) == 1
    ed.scheduler.set_timesteps(a["for_steps"], device=DEV)
    assert net.pullbacks[0][1][0] == float(ed.scheduler.timesteps[f["h_t_idx"]])
    names = [f"{p}xt-{a['dataset_name']}_{i}-{a['h_t']}T-mid-block_0-seed_{a['seed']}.pt" for i in (0, 1) for p in ("u-", "s-", "vT-")]
    assert sorted(x for x in os.listdir(save_dir) if x.endswith(".pt")) == sorted(names)
    u0 = torch.load(os.path.join(save_dir, names[0]))
    assert tuple(u0.shape) == tuple(f["u"][0].shape)
    ref = dict(f["saved"])["vk-sample_idx_0_0-sample_idx_1_1-pc_000.png"][0].reshape(1, -1)
    cos = abs_cos(out["vk"][0, 0].reshape(1, -1), ref).item()
    print("from-scratch bases: |cos| of the leading transported direction against the reference's", cos,
          "; per basis vector |cos| of vT", [abs_cos(torch.load(os.path.join(save_dir, names[3 * i + 2])), f["vT"][i]).tolist() for i in (0, 1)])
    assert cos >= 0.99
    assert sorted(n for n, _ in _pictures(saved)) == sorted(n for n, _ in _pictures(f["saved"]))
    assert all(torch.isfinite(x).all() for _, x in saved)


def test_a_list_of_targets_runs_the_source_once(fix, together, tmp_path):
    """targets [1, 2] (2: the mirror image of sample 0, its basis computed here): every target's names, ONE transport call with D = 2, the original-direction
    chains once; target 1's pictures are those of its single-target run"""
    f, a = fix, fix["args"]
    net, saved, out, ed, save_dir = _run(f, tmp_path, trajectory_batch=20, max_batch=20, max_rank=4, targets=[1, 2], vis_num_pc=1,
                                         extra={2: f["x0"][0].flip(-1).clone()})
    assert net.transports == [(2, 4, f["u"][0].shape[0])] and net.pullbacks == [(1, net.pullbacks[0][1])]
    assert tuple(out["vk"].shape) == (2, 1, 3 * 32 * 32) and out["targets"] == [1, 2]
    stem = "xt-CelebA_HQ-sample_idx_0_0-sample_idx_1_{}-h_0.8T-edit_0.6T-mid-block_0-seed_0-pc_000_{}"
    want = [stem.format(j, s) for j in (1, 2, 0) for s in ("pos", "neg")]
    assert out["names"] == want
    pics = _pictures(saved)
    assert sorted(n for n, _ in pics) == sorted([f"x0_gen-{n}.png" for n in want] + [f"vk-sample_idx_0_0-sample_idx_1_{j}-pc_000.png" for j in (1, 2)])
    got = dict(pics)
    assert got["vk-sample_idx_0_0-sample_idx_1_2-pc_000.png"].shape[0] == 4
    assert torch.equal(got["vk-sample_idx_0_0-sample_idx_1_1-pc_000.png"][2:], got["vk-sample_idx_0_0-sample_idx_1_2-pc_000.png"][2:])      # the source's own
    assert [c[1].shape[0] for c in net.calls[-30:]] == [12] * 8 + [20, 10] * 11          # 6 chains: 12 rows per guidance step, 30 decode states
    single = dict(_pictures(together[1]))
    assert torch.equal(out["vk"][0, 0], together[2]["vk"][0, 0])                        # a target's direction is the same alone and in the stack
    for n, x in pics:
        if "sample_idx_1_2" not in n:
            assert rel(x, single[n]) < TOL, n
    assert all(torch.isfinite(x).all() for _, x in saved)


def test_adm_kind_smoke(tmp_path, monkeypatch):
    """the same surface on the guided-diffusion family: the toy ADM net of --net_scale small, sized by main.build_unet for the job"""
    from diffusion_pullback_amd import edit as E
    from diffusion_pullback_amd import main as m
    argv = ["--note", "t", "--model_name", "FFHQ_P2", "--dataset_name", "Random", "--result_folder", str(tmp_path), "--device", DEV, "--net_scale", "small",
            "--performance_boosting_t", "0.2", "--x_space_guidance_scale", "0.1", "--x_space_guidance_num_step", "4", "--edit_t", "0.6", "--h_t", "0.8",
            "--run_edit_parallel_transport", "True", "--sample_idx_0", "0", "--sample_idx_1", "1", "--pca_rank", "3", "--vis_num_pc", "1"]
    args = m.preset(m.parse_args(argv))
    args.for_steps = args.inv_steps = 20
    args.input_root = os.path.join(str(tmp_path), "inputs")
    unet = m.build_unet(args)
    assert unet.kind == "adm" and unet.engine.max_batch >= 8 and unet.max_rank >= 6      # the chain call and the basis group of two
    saved = []
    monkeypatch.setattr(E, "save_image", lambda x, path, nrow=None: saved.append((os.path.basename(path), x.detach().float().cpu().clone())))
    ed = E.EditUncondDiffusion(args, unet=unet)
    out = ed.run_edit_parallel_transport(0, 1, op="mid", block_idx=0, vis_num=4, vis_num_pc=1, pca_rank=3)
    assert len(out["names"]) == 4 and torch.isfinite(out["vk"]).all() and torch.isfinite(out["coef_norm"]).all()
    assert [n for n, _ in saved] == [f"x0_gen-{n}.png" for n in out["names"]] + ["vk-sample_idx_0_0-sample_idx_1_1-pc_000.png"]
    assert all(tuple(x.shape) == (5, 3, 32, 32) and torch.isfinite(x).all() for n, x in saved if n.startswith("x0_gen-"))
    assert tuple(saved[-1][1].shape) == (4, 3, 32, 32) and torch.isfinite(saved[-1][1]).all()
    d = os.path.join(args.input_root, "local_encoder_pullback_uncond-model_FFHQ_P2-dataset_Random-num_steps_20-pca_rank_3")
    assert sorted(x for x in os.listdir(d) if x.endswith(".pt")) == sorted(f"{p}xt-Random_{i}-0.8T-mid-block_0-seed_0.pt" for i in (0, 1) for p in ("u-", "s-", "vT-"))
