"""run_tangent_space_pga end to end on the toy nets of both drivers (Stable Diffusion and the unconditional DDPM), through the CLI entry.  The sampling
job's files are staged, not sampled: planted bases (tests/_pga_ref.py) written under the names and in the directory that job uses, so that the set is
inside the log map's domain by construction and the job under test samples nothing."""
import os
import re

import numpy as np
import pytest
import torch

import _pga_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
K, N, PER = 3, 48, 4


def _argv(tmp, kind, *more):
    common = ["--note", "t", "--result_folder", str(tmp), "--device", DEV, "--net_scale", "small", "--pca_rank", str(K), "--num_local_basis", str(PER),
              "--dataset_name", "Random", *more]
    if kind == "sd":
        return common + ["--model_name", "runwayml/stable-diffusion-v1-5", "--edit_prompt", "tiger", "--for_steps", "20", "--inv_steps", "20"]
    return common + ["--model_name", "CelebA_HQ_HF", "--performance_boosting_t", "0.2"]


def _stage(root, kind):
    """vT- files of PER latents at h_t = 0.8 and 0.5 in the sampling job's directory, in its order (h_t outer); the first planted mode is linear in h_t"""
    if kind == "sd":
        d = os.path.join(root, f"local_encoder_pullback_stable_diffusion-dataset_Random-num_steps_20-pca_rank_{K}")
        name = lambda i, ht: f'zt-Random_{i}-{ht}T-"tiger"-mid-block_0-seed_0'
    else:
        d = os.path.join(root, f"local_encoder_pullback_uncond-model_CelebA_HQ_HF-dataset_Random-num_steps_100-pca_rank_{K}")
        name = lambda i, ht: f"xt-Random_{i}-{ht}T-mid-block_0-seed_0"
    os.makedirs(d, exist_ok=True)
    hts = [0.8] * PER + [0.5] * PER
    a, _, _, _ = R.planted_set(np.random.default_rng(11), 2 * PER, K, N, 2, noise=5e-2, covariate=np.array(hts))
    names = [name(i % PER, ht) for i, ht in enumerate(hts)]
    for nm, x in zip(names, a):
        torch.save(torch.tensor(x), os.path.join(d, "vT-" + nm + ".pt"))
    return d, names, hts


@pytest.mark.parametrize("kind", ["sd", "ddpm"])
def test_pga_job_end_to_end(tmp_path, kind, monkeypatch):
    from diffusion_pullback_amd import geometry
    from diffusion_pullback_amd import main as m
    root = os.path.join(str(tmp_path), "inputs")
    real_preset = m.preset

    def preset(args):                             # the drivers' basis cache goes under the test's directory
        args = real_preset(args)
        args.input_root = root
        return args
    monkeypatch.setattr(m, "preset", preset)
    d, names, hts = _stage(root, kind)
    base_keys = {"names", "idx", "h_t", "base", "modes", "variance", "explained", "scores", "residual", "theta", "mean_tangent_norm"}
    # two timesteps: the trend is fitted
    ed = m.main(_argv(tmp_path, kind, "--run_tangent_space_pga", "True", "--pga_base", "flag", "--pga_modes", "2", "--h_t_list", "0.8,0.5"))
    path = os.path.join(d, ed.EXP_NAME)
    assert ed.EXP_NAME.startswith("tangent_space_pga-x-flag-M2-") and "0to3" in ed.EXP_NAME and "0.8,0.5" in ed.EXP_NAME and os.path.exists(path + ".pt")
    try:
        import matplotlib                         # noqa: F401  (the plots are written only where matplotlib is installed)
        assert os.path.exists(path + "-scree.png") and os.path.exists(path + "-scores.png")
    except ImportError:
        pass
    out = torch.load(path + ".pt", weights_only=False)
    assert set(out) == base_keys | {"slopes", "intercept", "r2", "slope_norm"}
    assert out["names"] == names and out["idx"] == [0, 1, 2, 3] * 2 and out["h_t"] == hts
    stack = torch.stack([torch.load(os.path.join(d, "vT-" + n + ".pt"), map_location=DEV).float() for n in out["names"]])
    y, modes, info = geometry.grassmann_pga(stack, base="flag", n_modes=2, covariates=hts)
    assert torch.equal(info["scores"].cpu(), out["scores"]) and torch.equal(y.cpu(), out["base"]) and torch.equal(modes.cpu(), out["modes"])
    assert tuple(out["modes"].shape) == (2, K, N) and tuple(out["scores"].shape) == (2 * PER, 2) and tuple(out["slopes"].shape) == (1, K, N)
    assert tuple(out["intercept"].shape) == (K, N) and tuple(out["theta"].shape) == (2 * PER, K) and tuple(out["residual"].shape) == (2 * PER,)
    assert out["r2"] == info["r2"] and 0.3 < out["r2"] <= 1.0 and float(out["explained"][-1]) > 0.9       # the planted trend carries the first mode
    # one timestep: no trend fields; the default number of modes, the Karcher mean as the base
    ed = m.main(_argv(tmp_path, kind, "--run_tangent_space_pga", "True", "--h_t", "0.8"))
    assert ed.EXP_NAME.startswith("tangent_space_pga-x-frechet-M3-")
    out = torch.load(os.path.join(d, ed.EXP_NAME + ".pt"), weights_only=False)
    assert set(out) == base_keys and out["names"] == names[:PER] and out["h_t"] == [0.8] * PER
    y, modes, info = geometry.grassmann_pga(stack[:PER], base="frechet")
    assert torch.equal(info["scores"].cpu(), out["scores"]) and torch.equal(y.cpu(), out["base"]) and tuple(out["modes"].shape) == (3, K, N)
    os.remove(os.path.join(d, "vT-" + names[3] + ".pt"))
    with pytest.raises(ValueError, match=re.escape("vT-" + names[3] + ".pt")):
        m.main(_argv(tmp_path, kind, "--run_tangent_space_pga", "True", "--h_t", "0.8"))
