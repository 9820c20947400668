"""run_geodesic_interpolation on the HIP engine, on the small synthetic nets of main.build_unet: the unconditional driver and the Stable Diffusion one
(with the synthetic VAE).  m = 3 interior points, max_iter 4, 10 DDIM steps: the three pictures and the record under the stated names, the geodesic no
longer than the slerp curve it started from, the end rows of all three curves bitwise the two x_t, and a second run that loads the record without a
single U-Net call."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M, H_T = 3, 0.6
KINDS = ("lerp", "slerp", "geodesic")


class _Count:
    """counts the U-Net calls and the geodesic calls of a driver run; everything else is delegated to the wrapped PullbackUNet"""

    def __init__(self, net):
        self._net, self.calls = net, 0

    def __call__(self, *a, **k):
        self.calls += 1
        return self._net(*a, **k)

    def pullback_geodesic(self, *a, **k):
        self.calls += 1
        return self._net.pullback_geodesic(*a, **k)

    def curve_energy(self, *a, **k):
        self.calls += 1
        return self._net.curve_energy(*a, **k)

    def __getattr__(self, n):
        return getattr(self._net, n)


def _driver(model, tmp, net=None):
    from diffusion_pullback_amd import edit as E
    from diffusion_pullback_amd import main as m
    sd = "stable-diffusion" in model
    argv = ["--note", "t", "--model_name", model, "--dataset_name", "Random", "--result_folder", str(tmp), "--device", DEV, "--net_scale", "small",
            "--run_geodesic_interpolation", "True", "--sample_idx_0", "0", "--sample_idx_1", "1", "--geodesic_points", str(M), "--geodesic_max_iter", "4",
            "--h_t", str(H_T), "--seed", "3"] + (["--vae", "synthetic", "--for_steps", "10", "--inv_steps", "10"] if sd else ["--performance_boosting_t", "0.2"])
    args = m.preset(m.parse_args(argv))
    args.for_steps = args.inv_steps = 10
    args.input_root = os.path.join(str(tmp), "inputs")
    net = m.build_unet(args) if net is None else net
    assert net.engine.max_batch >= M + 2 and net.engine.max_tangents >= M
    args.image_size = net.in_shape[-1]
    if sd:
        return E.EditStableDiffusion(args, unet=_Count(net), vae=m.build_vae(args)), net
    ed = E.EditUncondDiffusion(args, unet=_Count(net))
    ed.performance_boosting_t_idx = 1000                   # the eta = 1 tail of the decode draws device noise
    return ed, net


@pytest.mark.parametrize("model", ["CelebA_HQ_HF", "runwayml/stable-diffusion-v1-5"])
def test_job_files_energies_end_rows_and_the_skip_rule(model, tmp_path, capsys):
    ed, net = _driver(model, tmp_path)
    rec = ed.run_geodesic_interpolation(sample_idx_0=0, sample_idx_1=1, op="mid", block_idx=0, h_t=H_T, n_points=M, max_iter=4)
    name = f"Geodesic-Random_0_1-{H_T}T-mid-block_0"
    assert rec["names"] == [f"{name}-{k}" for k in KINDS] and rec["seed"] == 3 and rec["n_points"] == M
    for k in KINDS:
        assert os.path.exists(os.path.join(ed.result_folder, f"x0_gen-{name}-{k}.png")), k
        assert tuple(rec["curves"][k].shape) == (M + 2, *net.in_shape) and torch.isfinite(rec["curves"][k]).all()
        assert all(key in rec["stats"][k] for key in ("energy", "energy_h", "energy_x", "length_h", "length_x", "uniformity", "seg_h", "seg_x"))
    path = os.path.join(ed.obs_folder, f"geodesic-{name}.pt")
    assert os.path.exists(path)
    out = capsys.readouterr().out
    assert all(f"{name} {k}: energy" in out for k in KINDS)
    s = rec["stats"]
    print({k: (s[k]["energy"], s[k]["length_h"], s[k]["uniformity"]) for k in KINDS}, rec["info"]["decisions"])
    assert s["geodesic"]["energy"] <= s["slerp"]["energy"] and rec["info"]["start"]["energy"] == s["slerp"]["energy"]
    assert rec["info"]["attempted"] == 4 and rec["info"]["energy"][-1] == s["geodesic"]["energy"]
    # the two x_t, taken there the way the job does
    ed.scheduler.set_timesteps(ed.for_steps, device=ed.device)
    idx = int((ed.scheduler.timesteps - H_T * 1000).abs().argmin())
    ends = [ed.DDIMforwardsteps(ed._random_latent(i), t_start_idx=0, t_end_idx=idx)[0].float().cpu() for i in (0, 1)]
    assert rec["t"] == float(ed.scheduler.timesteps[idx]) and not torch.equal(ends[0], ends[1])
    for k in KINDS:
        assert torch.equal(rec["curves"][k][0], ends[0][0]) and torch.equal(rec["curves"][k][-1], ends[1][0]), k
    assert not torch.equal(rec["curves"]["lerp"][1], rec["curves"]["slerp"][1])
    # a second run, on a fresh driver over the same net: the record is loaded, nothing runs
    ed2, _ = _driver(model, tmp_path, net=net)
    before = net.engine.stats()
    again = ed2.run_geodesic_interpolation(sample_idx_0=0, sample_idx_1=1, op="mid", block_idx=0, h_t=H_T, n_points=M, max_iter=4)
    assert ed2.unet.calls == 0 and net.engine.stats() == before
    assert again["names"] == rec["names"] and all(torch.equal(again["curves"][k], rec["curves"][k]) for k in KINDS)
    assert again["stats"]["geodesic"]["energy"] == s["geodesic"]["energy"]
    with pytest.raises(ValueError, match="two different samples"):
        ed2.run_geodesic_interpolation(sample_idx_0=1, sample_idx_1=1, op="mid", block_idx=0)
