"""run_sample_encoder_local_tangent_space_zt (reference src/modules/edit.py:310-383, :1517-1599; src/main.py:45-91) on the reduced nets of the
command line (--net_scale small): files and names, the "already sampled" skip, each saved basis against the single-sample method at the same
(x_t, t), the fix_xt pairing and the CLI flags."""
import os

import pytest
import torch

from _util import abs_cos

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H_T = [0.8, 0.5]


def _argv(tmp, kind, *more):
    common = ["--note", "t", "--result_folder", str(tmp), "--device", DEV, "--net_scale", "small", "--pca_rank", "2", "--num_local_basis", "2",
              "--h_t_list", "0.8,0.5", "--dataset_name", "Random", *more]
    if kind == "sd":
        return common + ["--model_name", "runwayml/stable-diffusion-v1-5", "--edit_prompt", "tiger", "--for_steps", "20", "--inv_steps", "20"]
    return common + ["--model_name", "CelebA_HQ_HF", "--performance_boosting_t", "0.2"]


def _driver(tmp, kind, *more):
    from diffusion_pullback_amd import main as m
    from diffusion_pullback_amd.edit import EditStableDiffusion, EditUncondDiffusion
    a = m.preset(m.parse_args(_argv(tmp, kind, "--run_sample_encoder_local_tangent_space_zt", "True", *more)))   # (build_unet sizes the engine for the job)
    a.input_root = os.path.join(str(tmp), "inputs")
    unet = m.build_unet(a)
    unet.verbose = False
    return a, (EditStableDiffusion if kind == "sd" else EditUncondDiffusion)(a, unet=unet)


class _Count:
    """counts every use of the U-Net (calls and bound methods); everything is delegated to the wrapped PullbackUNet"""

    def __init__(self, net):
        self._net, self.n = net, 0

    def __call__(self, *a, **k):
        self.n += 1
        return self._net(*a, **k)

    def __getattr__(self, name):
        v = getattr(self._net, name)
        if not callable(v):
            return v

        def f(*a, **k):
            self.n += 1
            return v(*a, **k)
        return f


def _close(got, ref, what):
    """the bar of test_batched_samples_match_single_sample_runs (fp32 engines): s rtol 1e-4, |cos| > 0.9999"""
    (u, s, vT), (u1, s1, v1) = got, ref
    assert torch.allclose(s.cpu(), s1.cpu(), rtol=1e-4), (what, s, s1)
    assert (abs_cos(vT, v1) > 0.9999).all() and (abs_cos(u.T, u1.T) > 0.9999).all(), what


@pytest.mark.parametrize("kind", ["sd", "ddpm"])
def test_tangent_space_driver_files_skip_and_bases(tmp_path, kind):
    a, ed = _driver(tmp_path, kind)
    unet = ed.unet
    assert unet.engine.max_batch >= 4 and unet.max_rank >= 8                  # build_unet sized the engine for the group of 2 x 2 pairs
    torch.manual_seed(11)                                                     # V0 of the batch method: one CPU draw per sample, in pair order
    ed.run_sample_encoder_local_tangent_space_zt(h_t=H_T, op="mid", block_idx=0, pca_rank=2, num_local_basis=2)
    if kind == "sd":
        d = os.path.join(a.input_root, "local_encoder_pullback_stable_diffusion-dataset_Random-num_steps_20-pca_rank_2")
        name = lambda i, ht: f'zt-Random_{i}-{ht}T-"tiger"-mid-block_0-seed_0'
    else:
        d = os.path.join(a.input_root, "local_encoder_pullback_uncond-model_CelebA_HQ_HF-dataset_Random-num_steps_100-pca_rank_2")
        name = lambda i, ht: f"xt-Random_{i}-{ht}T-mid-block_0-seed_0"
    pairs = [(i, ht) for ht in H_T for i in range(2)]
    for i, ht in pairs:
        for pre in ("u-", "s-", "vT-"):
            assert os.path.exists(os.path.join(d, pre + name(i, ht) + ".pt")), (pre, i, ht)
    assert sorted(ed.last_tangent_inputs) == sorted(pairs)
    n_h = unet.engine.tap_numel(("mid", 0))
    torch.manual_seed(11)
    V0s = [torch.linalg.qr(torch.randn(unet.engine.n_in, 2, dtype=torch.float))[0].T for _ in pairs]
    for (i, ht), V0 in zip(pairs, V0s):
        got = [torch.load(os.path.join(d, pre + name(i, ht) + ".pt"), map_location=DEV) for pre in ("u-", "s-", "vT-")]
        assert tuple(got[0].shape) == (n_h, 2) and tuple(got[1].shape) == (2,) and tuple(got[2].shape) == (2, unet.engine.n_in)
        assert got[0].untyped_storage().nbytes() == got[0].numel() * 4        # the file holds this basis, not the group's
        x, t = ed.last_tangent_inputs[(i, ht)]
        assert abs(t - float(ed.scheduler.timesteps[(ed.scheduler.timesteps - ht * 1000).abs().argmin()])) < 1e-3
        if kind == "sd":
            ref = unet.local_encoder_pullback_zt(x, t, ed.edit_prompt_emb, op="mid", block_idx=0, pca_rank=2, chunk_size=5, min_iter=10, max_iter=50,
                                                 convergence_threshold=1e-3, V0=V0)
        else:
            ref = unet.local_encoder_pullback_xt(x, t, op="mid", block_idx=0, pca_rank=2, min_iter=10, max_iter=50, convergence_threshold=1e-4, V0=V0)
        _close(got, ref, (i, ht))
    # a second call finds every basis sampled: no inversion, no DDIM step, no pullback
    ed.unet = _Count(unet)
    ed.run_sample_encoder_local_tangent_space_zt(h_t=H_T, op="mid", block_idx=0, pca_rank=2, num_local_basis=2)
    assert ed.unet.n == 0 and ed.last_tangent_inputs == {}
    # ... and a float h_t with one more basis samples exactly the missing pair
    ed.run_sample_encoder_local_tangent_space_zt(h_t=0.8, op="mid", block_idx=0, pca_rank=2, num_local_basis=3)
    assert list(ed.last_tangent_inputs) == [(2, 0.8)] and os.path.exists(os.path.join(d, "s-" + name(2, 0.8) + ".pt"))


def test_fix_xt_pairs_the_noise_image_with_every_timestep(tmp_path):
    a, ed = _driver(tmp_path, "ddpm")
    ed.run_sample_encoder_local_tangent_space_zt(h_t=H_T, op="mid", block_idx=0, pca_rank=2, num_local_basis=2, fix_xt=True)
    d = os.path.join(a.input_root, "local_encoder_pullback_uncond-model_CelebA_HQ_HF-dataset_Random-num_steps_100-pca_rank_2-fix_xt")
    ts = {}
    for i in range(2):
        for ht in H_T:
            assert os.path.exists(os.path.join(d, f"vT-xt-Random_{i}-{ht}T-mid-block_0-seed_0.pt"))
            x, t = ed.last_tangent_inputs[(i, ht)]
            assert torch.equal(x, ed._random_latent(i))                       # x is x_T for every h_t
            ts[ht] = t
    assert ts[0.8] > ts[0.5] > 0                                              # ... at the timestep of h_t
    s8 = torch.load(os.path.join(d, "s-xt-Random_0-0.8T-mid-block_0-seed_0.pt"))
    s5 = torch.load(os.path.join(d, "s-xt-Random_0-0.5T-mid-block_0-seed_0.pt"))
    assert not torch.allclose(s8, s5, rtol=1e-4)                              # the same x at two timesteps: two tangent spaces
    with pytest.raises(AssertionError):
        ed.run_sample_encoder_local_tangent_space_zt(h_t=0.8, op="mid", block_idx=0, pca_rank=2, num_local_basis=1, fix_xt=True, fix_t=True)


def test_cli_flags_reach_the_driver(tmp_path, monkeypatch):
    from diffusion_pullback_amd import main as m
    from diffusion_pullback_amd.edit import EditUncondDiffusion
    seen = {}
    monkeypatch.setattr(EditUncondDiffusion, "run_sample_encoder_local_tangent_space_zt", lambda self, **kw: seen.update(kw, unet=self.unet))
    m.main(_argv(tmp_path, "ddpm", "--run_sample_encoder_local_tangent_space_zt", "True", "--fix_xt", "True"))
    unet = seen.pop("unet")
    assert seen == dict(h_t=[0.8, 0.5], op="mid", block_idx=0, pca_rank=2, num_local_basis=2, fix_xt=True, fix_t=False)
    assert unet.engine.max_batch >= 4 and unet.max_rank >= 8
    a = m.parse_args(["--note", "t", "--h_t", "0.6"])
    assert a.h_t_values == [0.6] and a.run_sample_encoder_local_tangent_space_zt is False and a.num_local_basis == 10
