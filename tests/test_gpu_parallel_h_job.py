"""The parallel-h edit (--edit_xt parallel-h) of the global-basis jobs on the HIP engine against the run recorded from the reference's own
run_edit_global_frechet_mean_zt (tests/golden/make_golden_parallel_h.py: edit_xt = 'parallel-h', space h, with and without the SEGA rule): every
U-Net input call by call and every picture at the bar of tests/test_gpu_transport_job.py (relative error < 2e-3), chains together against one at a
time; then the job's own behaviour -- the skip rule, space x refused, local_projection=False without any local-basis file, the chain records, the
Hungarian and flag-mean jobs through the same tail -- and the CLI end to end."""
import os

import pytest
import torch

from _util import load_golden, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-3
N_PRE = 26                     # 18 inversion steps and 8 steps to edit_t, one sample each


class _Rec:
    """records every U-Net call (t, input), every inv_jac_chain call (chains) and every local_encoder_pullback_batch call of a driver run"""

    def __init__(self, net):
        self._net, self.calls, self.chains, self.pullbacks = net, [], [], []

    def __call__(self, x, t, *a, **k):
        self.calls.append((float(t), x.detach().float().cpu().clone()))
        return self._net(x, t, *a, **k)

    def inv_jac_chain(self, **k):
        self.chains.append((int(k["x"].shape[0]), float(k["t"]), k["steps"], k["step_size"], k["sega_sigma"], list(k["dirs"]), list(k["signs"])))
        return self._net.inv_jac_chain(**k)

    def local_encoder_pullback_batch(self, samples, timesteps, *a, **k):
        self.pullbacks.append(int(samples.shape[0]))
        return self._net.local_encoder_pullback_batch(samples, timesteps, *a, **k)

    def __getattr__(self, n):
        return getattr(self._net, n)


@pytest.fixture(scope="module")
def fix():
    f = load_golden("parallel_h_uncond_small.pt")
    f["bases"] = load_golden("frechet_uncond_small.pt")            # the pre-placed bases, the sample and the toy net the maker ran on
    rows = torch.cat([load_golden(n) for n in f["trace_files"]])
    saved = load_golden("parallel_h_uncond_small.saved.pt")
    r0 = 0
    for run in ("plain", "sega"):
        r = f["runs"][run]
        n = sum(r["trace_batch"])
        r["trace_x"] = list(rows[r0:r0 + n].split(r["trace_batch"]))
        r["saved"] = saved[run]
        r0 += n
    assert r0 == rows.shape[0]
    return f


def _run(f, tmp, run="plain", trajectory_batch=1, local_projection=True, job="frechet", space="h", place_own=True, place_global=True, place_local=False):
    """one run of a global-basis job in parallel-h mode on the fixture's toy net.  Returns (recorder, save_image calls, return value, driver)."""
    from diffusion_pullback_amd import PullbackUNet, configs as cf
    from diffusion_pullback_amd import edit as E
    from diffusion_pullback_amd import main as m
    from oracle import unet_ddpm
    b, a = f["bases"], f["args"]
    cfg = unet_ddpm.DDPMConfig(**b["cfg"])
    params = cf.ddpm_init_params(cfg, seed=b["seed"], spectrum=cf.Spectrum(**b["spectrum"]))
    net = _Rec(PullbackUNet("ddpm", cfg, params, dtype=torch.float32, device=DEV, max_batch=10, max_rank=16, verbose=False))
    argv = ["--note", "t", "--model_name", a["model_name"], "--dataset_name", a["dataset_name"], "--result_folder", str(tmp), "--device", DEV,
            "--performance_boosting_t", "0.2", "--edit_t", str(a["edit_t"]), "--h_t", str(a["h_t"]), "--seed", str(a["seed"]),
            "--trajectory_batch", str(trajectory_batch), "--edit_xt", "parallel-h", "--x_edit_step_size", str(a["x_edit_step_size"]),
            "--use_sega_reg", str(run == "sega"), "--sega_reg_sigma", str(a["sega_reg_sigma"])]
    args = m.preset(m.parse_args(argv))
    args.for_steps = args.inv_steps = a["for_steps"]
    args.image_size = 32
    args.input_root = os.path.join(str(tmp), "inputs")
    ed = E.EditUncondDiffusion(args, unet=net, dataset={0: b["x0"]})
    ed.performance_boosting_t_idx = 1000                   # as in the fixture: the eta = 1 tail draws device noise
    assert int(ed.edit_t_idx) == f["edit_t_idx"] and float(ed.scheduler.timesteps[ed.edit_t_idx]) == f["edit_t"]
    k, n = a["pca_rank"], a["num_local_basis"]
    own_dir, own_name = ed._tangent_space_naming("mid", 0, k)
    if place_own:
        os.makedirs(own_dir, exist_ok=True)
        torch.save(b["own_u"], os.path.join(own_dir, f"u-{own_name(0, a['h_t'])}.pt"))
        torch.save(b["own_vT"], os.path.join(own_dir, f"vT-{own_name(0, a['h_t'])}.pt"))
    if place_local:
        local_dir, local_name = ed._tangent_space_naming("mid", 0, k, dataset_name="Random")
        os.makedirs(local_dir, exist_ok=True)
        for i in range(n):
            torch.save(b["local_u"][i], os.path.join(local_dir, f"u-{local_name(i, a['h_t'])}.pt"))
            torch.save(b["local_vT"][i], os.path.join(local_dir, f"vT-{local_name(i, a['h_t'])}.pt"))
    if place_global:
        basis_path = ed.global_frechet_mean_paths("mid", 0, k, n, space)[0]
        os.makedirs(os.path.dirname(basis_path), exist_ok=True)
        torch.save(b["global_u" if space == "h" else "global_v"], basis_path)
    saved = []
    keep = E.save_image
    E.save_image = lambda x, path, nrow=None: saved.append((os.path.basename(path), x.detach().float().cpu().clone()))
    kw = dict(op="mid", block_idx=0, vis_num=a["vis_num"], pca_rank=k, num_local_basis=n, local_projection=local_projection, vis_num_pc=a["vis_num_pc"])
    try:
        if job == "frechet":
            out = ed.run_edit_global_frechet_mean_zt(a["idx"], frechet_mean_space=space, **kw)
        elif job == "flag":
            out = ed.run_edit_global_flag_mean_zt(a["idx"], flag_mean_space=space, **kw)
        else:
            out = ed.run_edit_global_hungarian_mean_zt(a["idx"], hungarian_mean_space=space, **kw)
    finally:
        E.save_image = keep
    return net, saved, out, ed


@pytest.fixture(scope="module")
def runs(fix, tmp_path_factory):
    return {(r, tb): _run(fix, tmp_path_factory.mktemp(f"{r}{tb}"), r, trajectory_batch=tb) for r in ("plain", "sega") for tb in (1, 20)}


def _chain_records(ed, names):
    return [torch.load(os.path.join(ed.obs_folder, f"chain-{n}.pt")) for n in names]


@pytest.mark.parametrize("run", ["plain", "sega"])
def test_one_chain_at_a_time_matches_the_reference_call_by_call(fix, runs, run):
    """trajectory_batch = 1, the reference's order: all 48 U-Net inputs (18 inversion steps, 8 to edit_t, per chain 11 decode calls of the 5 states)
    and every picture, names and order included; the chain ran at the timestep, vis_num steps of x_edit_step_size / vis_num; under the SEGA rule
    the kept counts are the reference's (its elements are all 1e-4 clear of their thresholds)"""
    net, saved, out, ed = runs[(run, 1)]
    r, a = fix["runs"][run], fix["args"]
    assert out["names"] == r["names"] and out["vk"] is not None and net.pullbacks == []
    sigma = a["sega_reg_sigma"] if run == "sega" else None
    assert net.chains == [(1, fix["edit_t"], a["vis_num"], a["x_edit_step_size"] / a["vis_num"], sigma, [0], [s]) for s in (1.0, -1.0)]
    assert len(net.calls) == len(r["trace_t"]) == N_PRE + 2 * 11
    worst = 0.0
    for i, (t, x) in enumerate(net.calls):
        assert t == r["trace_t"][i], (i, t, r["trace_t"][i])
        assert x.shape == r["trace_x"][i].shape, (i, x.shape, r["trace_x"][i].shape)
        worst = max(worst, rel(x, r["trace_x"][i]))
    print(f"{run}: worst relative U-Net input error {worst:.2e}")
    assert worst < TOL
    assert [n for n, _ in saved] == [n for n, _ in r["saved"]]
    errs = {n: rel(x, w) for (n, x), (_, w) in zip(saved, r["saved"])}
    print("pictures:", {n[-22:]: f"{e:.2e}" for n, e in errs.items()})
    assert max(errs.values()) < TOL
    for rec, c in zip(_chain_records(ed, out["names"]), r["chains"]):
        assert rec["sega_kept"].tolist() == [float((v != 0).sum()) for v in c["vk"]]
    if os.path.isdir(ed.obs_folder):                          # (the plots are written only where matplotlib is installed)
        plots = sorted(n for n in os.listdir(ed.obs_folder) if n.startswith("projection_coeff-"))
        assert plots in ([], sorted(r["plots"]))


@pytest.mark.parametrize("run", ["plain", "sega"])
def test_chains_together_match_the_reference_and_the_sequential_run(fix, runs, run):
    """the default trajectory_batch: ONE inv_jac_chain call of both chains and one decode batch of 10 rows per step -- the reference's rows, chain by
    chain, and the pictures of the sequential run, all at the same bar"""
    net, saved, out, ed = runs[(run, 20)]
    seq = runs[(run, 1)]
    r, a = fix["runs"][run], fix["args"]
    assert len(net.chains) == 1 and net.chains[0][0] == 2 and net.chains[0][5:] == ([0, 0], [1.0, -1.0])
    assert [c[1].shape[0] for c in net.calls] == [1] * N_PRE + [10] * 11
    worst = 0.0
    for i in range(11):
        want = torch.cat([r["trace_x"][N_PRE + i], r["trace_x"][N_PRE + 11 + i]])
        assert net.calls[N_PRE + i][0] == r["trace_t"][N_PRE + i]
        worst = max(worst, rel(net.calls[N_PRE + i][1], want))
    print(f"{run}: together, worst relative decode input error {worst:.2e}")
    assert worst < TOL
    assert sorted(n for n, _ in saved) == sorted(n for n, _ in r["saved"])
    ref, one = dict(r["saved"]), dict(seq[1])
    for n, x in saved:
        assert rel(x, ref[n]) < TOL and rel(x, one[n]) < TOL, n
    for rec, rec1 in zip(_chain_records(ed, out["names"]), _chain_records(seq[3], seq[2]["names"])):
        assert rec["sega_kept"].tolist() == rec1["sega_kept"].tolist()
        assert torch.allclose(rec["h_shift"], rec1["h_shift"], rtol=TOL, atol=0) and torch.allclose(rec["norm"], rec1["norm"], rtol=TOL, atol=0)


def test_chain_records(fix, runs):
    """chain-<EXP_NAME>.pt: one entry per step, the shifts one per state; every chain moves h against its direction, further at every step"""
    a = fix["args"]
    for key, (net, saved, out, ed) in runs.items():
        assert len(out["chains"]) == 2
        for rec, ret in zip(_chain_records(ed, out["names"]), out["chains"]):
            assert sorted(rec) == ["h_dist", "h_shift", "norm", "sega_kept", "sega_std"]
            assert all(rec[k].shape == (a["vis_num"],) for k in ("norm", "sega_kept", "sega_std"))
            assert all(rec[k].shape == (a["vis_num"] + 1,) for k in ("h_shift", "h_dist"))
            assert all(torch.equal(rec[k], ret[k]) for k in rec)
            assert rec["h_shift"][0] == 0 and (rec["h_shift"][1:] < 0).all() and (rec["h_shift"].diff() < 0).all(), (key, rec["h_shift"])
            assert (rec["norm"] > 0).all() and (rec["h_dist"][1:] >= rec["h_shift"][1:].abs()).all()
            if key[0] == "sega":
                assert (rec["sega_kept"] < 0.4 * 3072).all() and (rec["sega_std"] > 0).all()
            else:
                assert (rec["sega_kept"] == 3072).all() and (rec["sega_std"] == 0).all()


def test_a_finished_job_does_nothing_and_a_finished_experiment_is_skipped(fix, tmp_path):
    net, saved, out, ed = _run(fix, tmp_path, "plain", trajectory_batch=20)
    a = fix["args"]
    kw = dict(vis_num=a["vis_num"], pca_rank=a["pca_rank"], num_local_basis=a["num_local_basis"], frechet_mean_space="h", vis_num_pc=1)
    pos, neg = [os.path.join(ed.result_folder, f"x0_gen-{n}.png") for n in out["names"]]
    open(pos, "w").close()                                    # (save_image was captured: put the picture where the job looks for it)
    calls = len(net.calls)
    again = ed.run_edit_global_frechet_mean_zt(a["idx"], **kw)
    assert again["names"] == out["names"][1:] and net.chains[-1][0] == 1 and net.chains[-1][6] == [-1.0]      # only the _neg chain ran
    open(neg, "w").close()
    calls = len(net.calls)
    assert ed.run_edit_global_frechet_mean_zt(a["idx"], **kw) is None and len(net.calls) == calls


def test_space_x_is_refused_before_anything_runs(fix, tmp_path):
    with pytest.raises(ValueError, match="parallel-h"):
        _run(fix, tmp_path, "plain", space="x")
    for job in ("flag", "hungarian"):
        with pytest.raises(ValueError, match="parallel-h"):
            _run(fix, tmp_path, "plain", job=job, space="x", place_global=False)


def test_without_local_projection_no_local_basis_is_touched(fix, runs, tmp_path):
    """local_projection=False: allowed in this mode, the sample's own basis is neither read (none is there) nor sampled and written; the chains and
    pictures are those of the run with the projection, bit for bit (it only feeds the plot)"""
    net, saved, out, ed = _run(fix, tmp_path, "sega", trajectory_batch=20, local_projection=False, place_own=False)
    own_dir = ed._tangent_space_naming("mid", 0, fix["args"]["pca_rank"])[0]
    assert os.listdir(own_dir) == [] and net.pullbacks == [] and out["vk"] is None       # (the directory itself is made where its file names are formed)
    assert not any(n.startswith("projection_coeff-") for n in os.listdir(ed.obs_folder))
    want = runs[("sega", 20)]
    assert out["names"] == want[2]["names"] and [n for n, _ in saved] == [n for n, _ in want[1]]
    assert all(torch.equal(x, w) for (_, x), (_, w) in zip(saved, want[1]))
    # an own basis that IS there is still not read: a file that cannot be loaded does no harm
    for tag in ("u", "vT"):
        open(os.path.join(own_dir, f"{tag}-{ed._tangent_space_naming('mid', 0, 4)[1](0, fix['args']['h_t'])}.pt"), "w").close()
    for n, _ in saved:
        assert not os.path.exists(os.path.join(ed.result_folder, n))
    again = _run(fix, tmp_path, "sega", trajectory_batch=20, local_projection=False, place_own=False)
    assert all(torch.equal(x, w) for (_, x), (_, w) in zip(again[1], want[1]))


@pytest.mark.parametrize("job", ["flag", "hungarian"])
def test_the_other_global_basis_jobs_reach_the_same_tail(fix, tmp_path, job):
    """the flag-mean and the Hungarian job compute their own h-space basis from the four pre-placed local bases and hand it to the same chains"""
    net, saved, out, ed = _run(fix, tmp_path, "plain", trajectory_batch=20, local_projection=False, job=job, place_own=False, place_global=False,
                               place_local=True)
    a = fix["args"]
    assert len(out["names"]) == 2 and len(net.chains) == 1 and net.chains[0][:4] == (2, fix["edit_t"], a["vis_num"], a["x_edit_step_size"] / a["vis_num"])
    pics = [(n, x) for n, x in saved if n.startswith("x0_gen-")]                              # (the inversion saves its own two pictures first)
    assert sorted(n for n, _ in pics) == sorted(f"x0_gen-{n}.png" for n in out["names"])
    assert all(torch.isfinite(x).all() and tuple(x.shape) == (a["vis_num"] + 1, 3, 32, 32) for _, x in pics)
    for rec in _chain_records(ed, out["names"]):
        assert (rec["h_shift"][1:] < 0).all() and (rec["h_shift"].diff() < 0).all()


def test_cli_end_to_end_on_synthetic_weights(tmp_path, monkeypatch):
    """--run_edit_global_frechet_mean_zt True --frechet_mean_space h --edit_xt parallel-h --local_projection False --net_scale small: the engine sized
    by main.build_unet for the four chains of one call, the u- file, the pictures and the chain records"""
    from diffusion_pullback_amd import main as m
    monkeypatch.chdir(tmp_path)
    preset = m.preset

    def short(args):                                       # 20 DDIM steps instead of the preset's 100: the toy run stays within seconds
        args = preset(args)
        args.for_steps = args.inv_steps = 20
        return args
    monkeypatch.setattr(m, "preset", short)
    argv = ["--note", "t", "--model_name", "CelebA_HQ_HF", "--dataset_name", "Random", "--result_folder", str(tmp_path / "runs"), "--device", DEV,
            "--net_scale", "small", "--performance_boosting_t", "0.2", "--edit_t", "0.6", "--h_t", "0.8", "--run_edit_global_frechet_mean_zt", "True",
            "--frechet_mean_space", "h", "--num_local_basis", "4", "--pca_rank", "3", "--vis_num_pc", "2", "--vis_num", "3", "--frechet_max_iter", "200",
            "--edit_xt", "parallel-h", "--x_edit_step_size", "6", "--use_sega_reg", "True", "--sega_reg_sigma", "0.5", "--local_projection", "False"]
    ed = m.main(argv)
    assert ed.edit_xt == "parallel-h" and ed.unet.engine.max_batch >= 4 and ed.unet.max_rank >= 4
    assert os.path.basename(ed.global_frechet_mean_paths("mid", 0, 3, 4, "h")[0]) == "u-0.8T-mid-block_0-seed_0-num_local_basis_4.pt"
    stem = "xt-Random_0-h_0.8T-edit_0.6T-mid-block_0-seed_0-pc_00"
    names = [stem + s for s in ("0_neg", "0_pos", "1_neg", "1_pos")]
    assert sorted(x for x in os.listdir(ed.result_folder) if x.startswith("x0_gen-")) == [f"x0_gen-{n}.png" for n in names]
    assert sorted(x for x in os.listdir(ed.obs_folder) if x.startswith("chain-")) == [f"chain-{n}.pt" for n in names]
    for rec in _chain_records(ed, names):
        assert rec["norm"].shape == (3,) and (rec["h_shift"][1:] < 0).all() and (rec["sega_kept"] < 3 * 32 * 32).all() and (rec["sega_kept"] > 0).all()
