"""The newton-h edit (--edit_xt newton-h) of the global-basis jobs on the toy driver of tests/test_gpu_parallel_h_job.py: the files and the record keys,
the skip rule on a second run, the sign of the pos and neg chains, local_projection=False without any local-basis file, chains together against one
at a time, and every refusal before a pass runs."""
import os

import pytest
import torch

from _util import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H_STEP = 3.0


class _Rec:
    """records every U-Net call and every newton_h_chain call of a driver run"""

    def __init__(self, net):
        self._net, self.calls, self.chains = net, [], []

    def __call__(self, x, t, *a, **k):
        self.calls.append((float(t), int(x.shape[0])))
        return self._net(x, t, *a, **k)

    def newton_h_chain(self, **k):
        self.chains.append(dict(n=int(k["x"].shape[0]), t=float(k["t"]), steps=k["steps"], iters=k["iters"], scale=k["scale"], damping=k["damping"],
                                radius=k["radius"], dirs=list(k["dirs"]), signs=list(k["signs"])))
        return self._net.newton_h_chain(**k)

    def __getattr__(self, n):
        return getattr(self._net, n)


@pytest.fixture(scope="module")
def fix():
    f = load_golden("parallel_h_uncond_small.pt")
    f["bases"] = load_golden("frechet_uncond_small.pt")            # the pre-placed bases, the sample and the toy net
    return f


def _run(f, tmp, trajectory_batch=20, local_projection=False, job="frechet", space="h", extra=(), place_global=True, patch=None):
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
            "--trajectory_batch", str(trajectory_batch), "--edit_xt", "newton-h", "--h_edit_step_size", str(H_STEP), "--newton_iters", "3", *extra]
    args = m.preset(m.parse_args(argv))
    args.for_steps = args.inv_steps = a["for_steps"]
    args.image_size = 32
    args.input_root = os.path.join(str(tmp), "inputs")
    ed = E.EditUncondDiffusion(args, unet=net, dataset={0: b["x0"]})
    ed.performance_boosting_t_idx = 1000                   # as in the sibling's fixture: the eta = 1 tail draws device noise
    for k, v in (patch or {}).items():
        setattr(ed, k, v)
    k, n = a["pca_rank"], a["num_local_basis"]
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


def _records(ed, names):
    return [torch.load(os.path.join(ed.obs_folder, f"newton-{n}.pt")) for n in names]


KEYS = ["clip", "delta_norm", "h_dist", "h_off", "h_shift", "inner_iterations", "resid_norm", "scale"]


def test_files_records_and_signs(fix, tmp_path, capsys):
    """both chains through ONE newton_h_chain call from x_t at the timestep of edit_t, vis_num outer steps towards h_edit_step_size; the pictures
    under the sibling's names; newton-<name>.pt per chain; the pos chain moves h along u, and so does the neg chain along -u"""
    net, saved, out, ed = _run(fix, tmp_path)
    a = fix["args"]
    v = a["vis_num"]
    assert out["names"] == fix["runs"]["plain"]["names"] and out["vk"] is None
    assert net.chains == [dict(n=2, t=fix["edit_t"], steps=v, iters=3, scale=H_STEP, damping=0.1, radius=None, dirs=[0, 0], signs=[1.0, -1.0])]
    assert [n for n, _ in saved if n.startswith("x0_gen-xt")] == [f"x0_gen-{n}.png" for n in out["names"]]
    assert all(tuple(x.shape) == (v + 1, 3, 32, 32) and torch.isfinite(x).all() for n, x in saved if n.startswith("x0_gen-xt"))
    assert not any(n.startswith("projection_coeff-") for n in os.listdir(ed.obs_folder))
    recs = _records(ed, out["names"])
    for rec, ret in zip(recs, out["chains"]):
        assert sorted(rec) == KEYS and rec["scale"] == H_STEP
        assert all(rec[k].shape == (v + 1,) for k in ("h_shift", "h_dist", "h_off")) and all(rec[k].shape == (v,) for k in KEYS[:2] + KEYS[5:7])
        assert all(torch.equal(rec[k], ret[k]) for k in KEYS[:-1])
        assert rec["h_shift"][0] == 0 and (rec["h_shift"][1:] > 0).all() and (rec["h_shift"].diff() > 0).all(), rec["h_shift"]
        assert (rec["inner_iterations"] == 3).all() and (rec["clip"] == 1).all() and (rec["h_dist"][1:] >= rec["h_shift"][1:]).all()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("newton-h chain")]
    assert len(lines) == 2 and all("of 3 asked" in ln and "off-axis" in ln and "inner iterations" in ln for ln in lines)


def test_a_finished_experiment_is_skipped_and_a_finished_job_does_nothing(fix, tmp_path):
    net, saved, out, ed = _run(fix, tmp_path)
    a = fix["args"]
    kw = dict(vis_num=a["vis_num"], pca_rank=a["pca_rank"], num_local_basis=a["num_local_basis"], frechet_mean_space="h", vis_num_pc=1, local_projection=False)
    pos, neg = [os.path.join(ed.result_folder, f"x0_gen-{n}.png") for n in out["names"]]
    open(pos, "w").close()                                    # (save_image was captured: put the picture where the job looks for it)
    again = ed.run_edit_global_frechet_mean_zt(a["idx"], **kw)
    assert again["names"] == out["names"][1:] and net.chains[-1]["n"] == 1 and net.chains[-1]["signs"] == [-1.0]      # only the _neg chain ran
    open(neg, "w").close()
    calls, chains = len(net.calls), len(net.chains)
    assert ed.run_edit_global_frechet_mean_zt(a["idx"], **kw) is None and len(net.calls) == calls and len(net.chains) == chains


def test_one_chain_at_a_time_and_the_radius(fix, tmp_path):
    """trajectory_batch = 1: one call per experiment, the same shifts as together (another batch: close, not bitwise); --newton_radius clamps"""
    both = _run(fix, tmp_path / "a")
    net, saved, out, ed = _run(fix, tmp_path / "b", trajectory_batch=1)
    assert [c["n"] for c in net.chains] == [1, 1] and [c["signs"] for c in net.chains] == [[1.0], [-1.0]]
    for r1, r2 in zip(_records(ed, out["names"]), _records(both[3], both[2]["names"])):
        assert torch.allclose(r1["h_shift"], r2["h_shift"], rtol=2e-3, atol=0)
    net, saved, out, ed = _run(fix, tmp_path / "c", extra=("--newton_radius", "0.5"))
    assert net.chains[0]["radius"] == 0.5
    for rec in _records(ed, out["names"]):
        assert (rec["clip"] <= 1).all() and (rec["clip"] * rec["delta_norm"] <= 0.5 * (1 + 1e-12)).all()


@pytest.mark.parametrize("job", ["flag", "hungarian"])
def test_space_x_is_refused_before_anything_runs(fix, tmp_path, job):
    for j in ("frechet", job):
        with pytest.raises(ValueError, match="newton-h"):
            _run(fix, tmp_path, job=j, space="x", place_global=False)


def test_every_refusal_comes_before_a_pass(fix, tmp_path):
    """a driver whose settings were changed after the parser (which refuses them itself): no U-Net call, no chain"""
    class Never:
        def __getattr__(self, n):
            raise AssertionError(f"the job touched the net ({n}) before refusing")

    for patch, word in ((dict(h_edit_step_size=0.0), "h_edit_step_size"), (dict(edit_ht="h_space_guidance"), "exclude each other"),
                        (dict(newton_iters=-1), "newton_iters"), (dict(edit_xt="newton"), "newton-h")):
        with pytest.raises(ValueError, match=word):
            _run(fix, tmp_path, patch={**patch, "unet": Never()})
    from diffusion_pullback_amd import main as m
    with pytest.raises(SystemExit):
        m.parse_args(["--note", "t", "--model_name", "stable-diffusion-v1-5", "--edit_xt", "newton-h", "--h_edit_step_size", "1"])
