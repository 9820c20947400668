"""The h-space guidance edit without a GPU: the float64 restatement of tests/_hguide_ref.py against its own identities, the bar of
tests/test_gpu_ddim_step_asym.py checked in numpy, the scheduler helper, the exported symbols and their host-side refusals, the command line.
(The kernels: tests/test_gpu_ddim_step_asym.py, tests/test_gpu_forward_shift_groups.py, tests/test_gpu_hguide_chain.py.)"""
import ctypes as C

import numpy as np
import pytest
import torch

import _hguide_ref as R
import test_gpu_ddim_step_asym as T


def _toy(seed=0, n=3, N=20):
    g = torch.Generator().manual_seed(seed)
    x, e = torch.randn(n, N, generator=g, dtype=torch.float64), torch.randn(n, N, generator=g, dtype=torch.float64)
    return x, e, e + 0.3 * torch.randn(n, N, generator=g, dtype=torch.float64)


def test_reference_identities():
    """mode (1, 1) is the plain DDIM step on e_s; x' - x'_plain = coef d with the coefficient of dx_norm, for any g; d = 0 gives the plain step"""
    x, e, es = _toy()
    a, an = 0.3054, 0.3287
    plain = lambda ee: (an ** 0.5) * ((x - ee * (1 - a) ** 0.5) / a ** 0.5) + (1 - an) ** 0.5 * ee
    out, P, d = R.step_ref(x, e, es, a, an, 1.0, 1.0)
    assert torch.allclose(out, plain(es), rtol=0, atol=1e-14)
    for gP, gD in [(1.0, 0.0), (1.0, 1.0), (0.0, 0.0), (-2.5, 0.5)]:
        out, P, d = R.step_ref(x, e, es, a, an, gP, gD)
        coef = float(R.dx_coef(a, an, gP, gD))
        assert torch.allclose(out - plain(e), coef * d, rtol=0, atol=1e-13), (gP, gD)
        assert torch.allclose(P, (x - (e + gP * d) * (1 - a) ** 0.5) / a ** 0.5, rtol=0, atol=1e-14)
    assert abs(float(R.dx_coef(a, an, 1.0, 0.0)) + (an * (1 - a) / a) ** 0.5) < 1e-15 and float(R.dx_coef(a, an, 0.0, 0.0)) == 0.0
    out, _, d = R.step_ref(x, e, e, a, an, -2.5, 0.5)
    assert torch.equal(out, plain(e)) and not d.any()


def test_chain_ref_with_scale_zero_is_the_plain_chain():
    """a net whose shifted output is eps(x) + A shift: scale 0 gives the plain DDIM chain exactly, delta_norm = |scale| ||A c|| at every step, and
    dx_norm the coefficient times it"""
    g = torch.Generator().manual_seed(3)
    W, A = 0.1 * torch.randn(12, 12, generator=g, dtype=torch.float64), torch.randn(12, 5, generator=g, dtype=torch.float64)
    eps = lambda x, t: torch.tanh(x.flatten(1) @ W.T).reshape(x.shape) * (1 + t / 1000)
    eps_s = lambda x, t, shift: eps(x, t) + (shift @ A.T).reshape(x.shape)
    x = torch.randn(3, 3, 2, 2, generator=g, dtype=torch.float64)
    c = torch.randn(3, 5, generator=g, dtype=torch.float64)
    c = c / c.norm(dim=1, keepdim=True)
    ts, al, an = [696.0, 686.0, 676.0], [0.30, 0.32, 0.34], [0.32, 0.34, 0.36]
    scales = [0.0, 1.5, -2.0]
    r = R.chain_ref((eps, eps_s), x, c, scales, ts, al, an, 1.0, 0.0)
    cur = x[:1]
    for t, a, a2 in zip(ts, al, an):
        cur = R.step_ref(cur, eps(cur, t), eps(cur, t), a, a2, 1.0, 0.0)[0]
    assert torch.allclose(r["states"][0, -1], cur[0], rtol=0, atol=1e-13) and (r["delta_norm"][0] == 0).all()      # (a row alone and in a batch: BLAS may differ by an ulp)
    assert (r["dx_norm"][0] == 0).all()
    for b in (1, 2):
        want = abs(scales[b]) * (A @ c[b]).norm()
        assert torch.allclose(r["delta_norm"][b], want.expand(3), rtol=1e-12)
        coef = torch.stack([R.dx_coef(a, a2, 1.0, 0.0).abs() for a, a2 in zip(al, an)])
        assert torch.allclose(r["dx_norm"][b], coef * want, rtol=1e-12)
    zero = R.chain_ref((eps, eps_s), x, c, scales, ts, al, an, 0.0, 0.0)          # g = (0, 0): the shift has no effect on the states
    assert torch.equal(zero["states"][1], R.chain_ref((eps, eps_s), x, c, [0.0] * 3, ts, al, an, 0.0, 0.0)["states"][1])
    rs = R.resync_ref((eps, eps_s), r, c, scales, ts, al, an, 1.0, 0.0, torch.float64)
    assert torch.allclose(rs["states"], r["states"][:, 1:], rtol=0, atol=1e-6)     # (the restart goes through fp32 states)


def test_numpy_fp32_evaluation_within_the_unit():
    """the bar's own check: fp32 numpy in the kernel's order against float64, 200 random cases, worst ratio to the unit below 5.0 (the test's bar: 8)"""
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(200):
        a_t, a_n = np.float32(rng.uniform(0.01, 0.98)), np.float32(rng.uniform(0.02, 0.999))
        gP, gD = np.float32(rng.uniform(-3, 3)), np.float32(rng.uniform(-3, 3))
        x, e = rng.standard_normal(257).astype(np.float32), rng.standard_normal(257).astype(np.float32)
        es = (e + np.float32(0.3) * rng.standard_normal(257).astype(np.float32)).astype(np.float32)
        sa, s1a, san, s1an = T._coefs(a_t, a_n)
        d = es - e
        eP, eD = e + gP * d, e + gD * d
        out = san * ((x - eP * s1a) / sa) + s1an * eD
        assert out.dtype == np.float32
        ref, _, _, unit = T._ref64(x, e, es, a_t, a_n, gP, gD)
        worst = max(worst, float((np.abs(out - ref) / unit).max()))
    print("worst fp32 / unit", worst)
    assert worst < 5.0


def test_scheduler_ddim_triples_are_the_coefficients_of_step():
    from diffusion_pullback_amd.scheduler import YHCustomScheduler, extract
    s = YHCustomScheduler(noise_schedule="linear")
    with pytest.raises(ValueError):
        s.ddim_triples(0, 3)
    s.set_timesteps(100)
    ts, al, an = s.ddim_triples(30, 33)
    assert len(ts) == len(al) == len(an) == 3
    for j, i in enumerate(range(30, 33)):
        t, tn = s.timesteps[i], s.timesteps_next[i]
        assert ts[j] == float(t)
        assert al[j] == float(extract(s.alphas_cumprod, t.reshape(()), (1,)).item())          # the .long() truncation of step's own lookup
        assert an[j] == float(extract(s.alphas_cumprod, tn.reshape(()), (1,)).item())
        assert al[j] == float(s.alphas_cumprod[int(float(t))]) and 0 < al[j] < an[j] <= 1
    assert an[0] == al[1]                                                                     # consecutive steps share an entry of the table
    for bad in ((-1, 3), (5, 5), (7, 3), (0, 101)):
        with pytest.raises(ValueError):
            s.ddim_triples(*bad)


NAMES = ("dpb_ddim_step_asym", "dpb_ddim_step_asym_scratch_bytes", "dpb_forward_shift_groups", "dpb_hguide_chain", "dpb_hguide_chain_scratch_bytes")


def test_new_symbols_are_exported():
    import inspect
    import os
    from diffusion_pullback_amd import PullbackUNet, engine, lib
    from diffusion_pullback_amd.edit import EditUncondDiffusion
    for n in NAMES:
        assert n in lib.SYMBOLS, n
    L = lib.load()                                                # binds every declared symbol: a missing one raises
    assert L.dpb_abi_version() == 1
    assert L.dpb_ddim_step_asym_scratch_bytes(3, 4097) == 3 * 2 * 2 * 8 and L.dpb_ddim_step_asym_scratch_bytes(0, 5) == 0
    assert L.dpb_hguide_chain_scratch_bytes(None, 1, 1) == 0
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dpb.h")).read()
    for n in NAMES:
        assert n + "(" in header, n
    assert callable(engine.ddim_step_asym) and callable(engine.Engine.forward_shift_groups) and callable(engine.Engine.hguide_chain)
    sig = inspect.signature(PullbackUNet.h_space_guidance).parameters
    for a in ("x", "timesteps", "alphas", "alphas_next", "u", "dirs", "scales", "mode", "encoder_hidden_states", "op", "block_idx"):
        assert a in sig, a
    assert sig["mode"].default == "asyrp"
    assert hasattr(EditUncondDiffusion, "_run_h_guidance_chains")


def test_host_side_refusals_need_no_gpu():
    """the entry points validate their host arguments before anything is launched (device pointers: a dummy non-null value, never read)"""
    from diffusion_pullback_amd import lib
    L = lib.load()
    err = lambda: L.dpb_last_error()
    step = lambda **k: L.dpb_ddim_step_asym(k.get("x", 8), 8, 8, 8, None, k.get("n", 2), k.get("N", 4), k.get("a", 0.5), k.get("an", 0.6), k.get("gP", 1.0),
                                            k.get("gD", 0.0), 8, k.get("scratch", 256), k.get("bytes", 1 << 20), None)
    assert step(x=None) != 0 and b"null" in err()
    assert step(n=0) != 0 and b"n=0" in err()
    assert step(N=0) != 0 and b"row length 0" in err()
    for kw in (dict(a=float("nan")), dict(gP=float("inf")), dict(gD=float("nan")), dict(an=float("inf"))):
        assert step(**kw) != 0 and b"non-finite" in err(), kw
    for kw in (dict(a=0.0), dict(a=1.5), dict(an=-0.1), dict(an=1.0000001)):
        assert step(**kw) != 0 and b"(0, 1]" in err(), kw
    assert step(bytes=8) != 0 and b"scratch" in err()
    assert step(scratch=260) != 0 and b"aligned" in err()
    # the engine entry points refuse a null engine and null arrays before they touch anything
    d, f = (C.c_int32 * 2)(0, 0), (C.c_float * 2)(1.0, 1.0)
    assert L.dpb_forward_shift_groups(None, 8, 1, 2, 1.0, None, 0, 8, 1, d, f, 1, 3, 8) != 0 and b"null" in err()
    assert L.dpb_hguide_chain(None, 0, 1, 8, 1, f, f, f, None, 8, 1, d, f, 1.0, 0.0, 1, 8, 8, 8, 1 << 20) != 0 and b"null" in err()


def _parse(*argv):
    from diffusion_pullback_amd.main import parse_args
    return parse_args(["--note", "n", *argv])


JOB = ("--run_edit_global_frechet_mean_zt", "True", "--frechet_mean_space", "h", "--model_name", "CelebA_HQ_HF")


def test_edit_ht_flags_and_parser_errors(capsys):
    from diffusion_pullback_amd.main import _FLAGS
    a = _parse()
    assert (a.edit_ht, a.h_edit_step_size, a.no_edit_t, a.h_guidance_mode) == ("default", 0, 0.5, "asyrp")
    assert {"edit_ht", "h_edit_step_size", "no_edit_t", "h_guidance_mode"} <= {f[0] for f in _FLAGS}
    ok = _parse(*JOB, "--edit_ht", "h_space_guidance", "--h_edit_step_size", "2.5", "--no_edit_t", "0.6", "--h_guidance_mode", "symmetric")
    assert (ok.edit_ht, ok.h_edit_step_size, ok.no_edit_t, ok.h_guidance_mode, ok.edit_xt) == ("h_space_guidance", 2.5, 0.6, "symmetric", "parallel-x")
    assert _parse(*JOB, "--edit_ht", "h_space_guidance", "--h_edit_step_size", "-1").h_edit_step_size == -1
    g = ("--edit_ht", "h_space_guidance", "--h_edit_step_size", "1")
    for argv in (("--edit_ht", "multiple-t"), ("--h_guidance_mode", "other"), ("--edit_xt", "default"), (*g, "--edit_xt", "default"),
                 ("--edit_ht", "h_space_guidance"),                                                       # h_edit_step_size == 0
                 (*JOB, "--edit_ht", "h_space_guidance", "--h_edit_step_size", "0"),
                 (*JOB, *g, "--no_edit_t", "1.0"), (*JOB, *g, "--no_edit_t", "0.7", "--edit_t", "0.6"),   # no_edit_t_idx <= edit_t_idx
                 (*JOB, *g, "--performance_boosting_t", "0.2", "--no_edit_t", "0.1"),                     # reaches the eta = 1 steps
                 (*JOB, *g, "--edit_xt", "parallel-h", "--x_edit_step_size", "1"),
                 ("--run_edit_global_frechet_mean_zt", "True", "--frechet_mean_space", "x", "--model_name", "CelebA_HQ_HF", *g),     # space x
                 ("--run_edit_global_flag_mean_zt", "True", "--model_name", "CelebA_HQ_HF", *g),
                 ("--run_edit_global_hungarian_mean_zt", "True", "--model_name", "CelebA_HQ_HF", *g),
                 (*g, "--model_name", "stable-diffusion-v1-5")):
        with pytest.raises(SystemExit):
            _parse(*argv)
    capsys.readouterr()
    _parse(*JOB, *g, "--no_edit_t", "0.4", "--h_guidance_mode", "asyrp")
    assert "ignoring" not in capsys.readouterr().out                     # the flags are flags now: none is reported among the ignored ones
    # h_space_guidance lifts the local_projection rule of the h-space bases exactly as parallel-h does
    with pytest.raises(SystemExit):
        _parse(*JOB, "--local_projection", "False")
    assert _parse(*JOB, *g, "--local_projection", "False").local_projection is False
    for job, space in (("flag", "flag_mean_space"), ("hungarian", "hungarian_mean_space")):
        argv = (f"--run_edit_global_{job}_mean_zt", "True", f"--{space}", "h", "--model_name", "CelebA_HQ_HF", "--local_projection", "False")
        with pytest.raises(SystemExit):
            _parse(*argv)
        assert _parse(*argv, *g).edit_ht == "h_space_guidance"
    # the namespace: no derived attribute, the same keys with the flags given or not
    assert set(vars(_parse(*JOB))) == set(vars(_parse(*JOB, *g)))


def _driver(**kw):
    """EditUncondDiffusion on a namespace of the parser's defaults, without a U-Net: the job-level checks run before anything is computed"""
    import tempfile
    from diffusion_pullback_amd.edit import EditUncondDiffusion
    a = _parse("--model_name", "CelebA_HQ_HF", "--dataset_name", "Random", "--performance_boosting_t", "0.2")
    d = tempfile.mkdtemp()
    vars(a).update(dict(result_folder=d, obs_folder=d, device="cpu", dtype=torch.float32, edit_ht="h_space_guidance", h_edit_step_size=1.0), **kw)
    return EditUncondDiffusion(a, unet=None)


@pytest.mark.parametrize("kw,space,word", [
    (dict(), "x", "space 'h'"),
    (dict(h_edit_step_size=0.0), "h", "h_edit_step_size"),
    (dict(no_edit_t=1.0), "h", "no_edit_t_idx > edit_t_idx"),
    (dict(edit_t=0.5, no_edit_t=0.7), "h", "no_edit_t_idx > edit_t_idx"),
    (dict(no_edit_t=0.1), "h", "performance_boosting_t_idx"),
    (dict(edit_xt="parallel-h", x_edit_step_size=1.0), "h", "exclude each other"),
    (dict(edit_ht="single-t"), "h", "edit_ht must be"),
    (dict(h_guidance_mode="other"), "h", "h_guidance_mode"),
])
def test_job_level_rules_raise_before_anything_is_computed(kw, space, word):
    ed = _driver(**kw)
    for job, name in (("run_edit_global_frechet_mean_zt", "frechet_mean_space"), ("run_edit_global_flag_mean_zt", "flag_mean_space"),
                      ("run_edit_global_hungarian_mean_zt", "hungarian_mean_space")):
        with pytest.raises(ValueError, match=word):
            getattr(ed, job)(0, **{name: space})
    ok = _driver()
    ok._check_parallel_h("h")                                            # the default interval (edit_t 1.0 -> no_edit_t 0.5, boosting at 0.2) passes
    assert int(ok.no_edit_t_idx) > int(ok.edit_t_idx) and int(ok.no_edit_t_idx) <= int(ok.performance_boosting_t_idx)
