"""The parallel-h edit chain without a GPU: the float64 restatements of tests/_chain_ref.py against closed forms, the exported symbols, the
command line.  (The kernels themselves: tests/test_gpu_direction_step.py, tests/test_gpu_inv_jac_chain.py.)"""
import numpy as np
import pytest
import torch

import _chain_ref as R

EPS32 = 2.0 ** -24


def _linear(seed=0, D=7, N=12):
    g = np.random.default_rng(seed)
    A = g.standard_normal((D, N))
    return A, g.standard_normal(D), g.standard_normal(N).astype(np.float32)


def test_restatement_on_a_linear_map_is_the_straight_line():
    """h = A x: J^T c = A^T c at every state, so x_j = x_0 - j s A^T c^ / ||A^T c^|| and h_shift[j] = -j s ||A^T c^|| (c^ = c / ||c||).  Per step
    the restatement rounds v and x once each: |x_j - line| <= j (2^-24 |x| + s 2^-24 |v|) and a little for W's own rounding to fp32."""
    A, c, x0 = _linear()
    s, steps = 0.37, 5
    w = A.T @ c
    W = w.astype(np.float32)[None]
    vhat = -w / np.linalg.norm(w)
    x = x0[None].copy()
    u = c.astype(np.float32)[None]
    h0 = (A @ x0.astype(np.float64)).astype(np.float32)[None]
    for j in range(1, steps + 1):
        x, vk, stats, _ = R.direction_step_ref(W, x, [s])
        line = x0.astype(np.float64) + j * np.float64(np.float32(s)) * vhat
        assert np.all(np.abs(x[0] - line) <= j * 4 * EPS32 * (np.abs(line) + s)), j
        assert np.all(np.abs(vk[0] - vhat) <= 4 * EPS32 * np.abs(vhat) + 1e-12)
        assert stats[0, 3] == 0 and stats[0, 2] == W.shape[1] and stats[0, 1] == 0
        assert abs(np.sqrt(stats[0, 0]) - np.linalg.norm(w)) <= 1e-6 * np.linalg.norm(w)
        h = (A @ x[0].astype(np.float64)).astype(np.float32)[None]
        a, q = R.shift_stats_ref(h, h0, u, [0], [1.0])[0]
        chat = c / np.linalg.norm(c)
        want = -j * s * np.linalg.norm(A.T @ chat)
        assert abs(a - want) <= 1e-5 * abs(want) + 1e-5, (j, a, want)
        assert abs(np.sqrt(q) - j * s * np.linalg.norm(A @ vhat)) <= 1e-5 * j * s * np.linalg.norm(A @ vhat) + 1e-5
    # a negative sign turns the shift round and nothing else
    a2, q2 = R.shift_stats_ref(h, h0, u, [0], [-1.0])[0]
    assert a2 == -a and q2 == q


def test_chain_ref_on_a_linear_map_is_the_straight_line():
    """the autograd chain in float64 on h = A x: the same line to fp64 accuracy, norm = ||A^T c|| at every step, for both signs"""
    A, c, x0 = _linear(1, D=8, N=16)
    At = torch.tensor(A)
    get_h = lambda x: (x.reshape(1, -1) @ At.T).reshape(1, 8, 1, 1)
    x = torch.tensor(x0).reshape(1, 1, 4, 4).repeat(2, 1, 1, 1)
    cs = torch.stack([torch.tensor(c), -torch.tensor(c)])
    s, steps = 0.25, 4
    r = R.chain_ref([get_h, get_h], x, cs, steps, [s, s])
    w = A.T @ c
    for b, sg in enumerate((1.0, -1.0)):
        for j in range(steps + 1):
            line = x0.astype(np.float64) - sg * j * s * w / np.linalg.norm(w)
            assert np.allclose(r["states"][b, j].reshape(-1).numpy(), line, rtol=0, atol=1e-13)
            assert abs(float(r["h_shift"][b, j]) + j * s * np.linalg.norm(w) / np.linalg.norm(c)) < 1e-12
        assert np.allclose(r["norm"][b].numpy(), np.linalg.norm(w), rtol=1e-14)
        assert (r["sega_kept"][b] == 16).all() and (r["sega_std"][b] == 0).all()
    assert (r["h_shift"][:, 1:] < 0).all()                       # a + chain moves h AGAINST c


def test_sega_rule_on_rows_whose_kept_set_is_known():
    """w = (10, -10, 1, -1, 0.5, 0, 0, 0): unit-norm v has |v| = (10, 10, 1, 1, .5, 0, 0, 0) / sqrt(202.25); the mean is 0.5 / 8 / sqrt(202.25) and
    std = sqrt((1 - S1^2 / (N S2)) / (N - 1)) = 0.37789...; sigma = 1 keeps the two of size 0.70, sigma = 0.1 also the two of size 0.070 (threshold
    0.0378) and drops 0.035; sigma = 0.05 keeps five.  Zeros are never kept when the rule is on."""
    w = np.array([[10, -10, 1, -1, 0.5, 0, 0, 0]], np.float32)
    x = np.arange(8, dtype=np.float32)[None]
    nrm = np.sqrt(202.25)
    std = np.sqrt((1 - 0.25 / (8 * 202.25)) / 7)
    tstd = float(torch.tensor(-w[0].astype(np.float64) / nrm).std())
    assert abs(std - tstd) < 1e-15                               # the formula in the two sums IS torch's unbiased std of the unit-norm row
    for sigma, kept in ((1.0, [0, 1]), (0.1, [0, 1, 2, 3]), (0.05, [0, 1, 2, 3, 4])):
        xo, vk, stats, margin = R.direction_step_ref(w, x, [2.0], sigma)
        assert sorted(np.nonzero(vk[0])[0].tolist()) == kept, sigma
        assert stats[0, 2] == len(kept) and abs(stats[0, 1] - std) < 1e-15 and stats[0, 3] == 0
        assert np.array_equal(xo[0][[5, 6, 7]], x[0][[5, 6, 7]])
        assert np.allclose(xo[0][kept], x[0][kept] + 2.0 * (-w[0][kept] / nrm), rtol=1e-6)
        assert margin.min() > 1e-3
    xo, vk, stats, _ = R.direction_step_ref(w, x, [2.0], 0.0)     # off: every element kept, the zeros included
    assert stats[0, 2] == 8 and stats[0, 1] == 0


def test_n_equal_one_and_degenerate_rows():
    """N = 1: v = -sign(w) and the SEGA rule leaves it alone (the reference's std is NaN there and its where keeps the element).  A zero row and
    a row with an inf: flag and NaN in that row only."""
    xo, vk, stats, _ = R.direction_step_ref(np.array([[3.0], [-2.0]], np.float32), np.array([[1.0], [1.0]], np.float32), [0.5, 0.5], 1.0)
    assert vk[:, 0].tolist() == [-1.0, 1.0] and xo[:, 0].tolist() == [0.5, 1.5] and stats[:, 2].tolist() == [1, 1] and stats[:, 1].tolist() == [0, 0]
    v = torch.tensor([-1.0])
    assert torch.isnan(v.std()) and torch.where(v.abs() < 1.0 * v.std(), torch.zeros_like(v), v).item() == -1.0
    W = np.array([[1, 2, 2], [0, 0, 0], [1, np.inf, 0], [0, 3, 4]], np.float32)
    xo, vk, stats, _ = R.direction_step_ref(W, np.ones((4, 3), np.float32), [1.0] * 4)
    assert stats[:, 3].tolist() == [0, 1, 1, 0]
    assert np.isnan(xo[1]).all() and np.isnan(vk[2]).all() and np.isfinite(xo[[0, 3]]).all()
    assert np.allclose(vk[3], [0, -0.6, -0.8]) and np.allclose(xo[0], 1 - np.array([1, 2, 2]) / 3.0)


@pytest.mark.parametrize("run", ["plain", "sega"])
def test_restatement_against_the_reference_run(run):
    """The fixture of tests/golden/make_golden_parallel_h.py: the reference's own parallel-h branch.  Fed with W = -v_raw (the reference's unit
    direction) and the reference's state, the restatement gives the reference's v_k -- the same elements cut, the others within
    delta + 2 * 2^-24 relative, delta = |1 - ||v_raw||| being what the reference's fp32 norm left its "unit" row short of 1 (read off the
    fixture: about 4e-7), the rest two roundings -- and its next state within the roundings of x + s v (the reference forms s v and the sum in
    fp32: 2^-24 of each, on top of v's own error)."""
    from _util import load_golden
    f = load_golden("parallel_h_uncond_small.pt")
    a = f["args"]
    s = a["x_edit_step_size"] / a["vis_num"]
    sigma = a["sega_reg_sigma"] if run == "sega" else 0.0
    assert a["turn"] < 0.99 and a["sega_margin"] >= 1e-4 and len(f["runs"][run]["chains"]) == 2
    for c in f["runs"][run]["chains"]:
        n = a["vis_num"]
        W = (-c["v_raw"]).numpy()
        x = c["states"][:n].reshape(n, -1).numpy()
        xo, vk, stats, margin = R.direction_step_ref(W, x, [s] * n, sigma)
        want_v, want_x = c["vk"].numpy().astype(np.float64), c["states"][1:].reshape(n, -1).numpy().astype(np.float64)
        assert np.array_equal(vk == 0, want_v == 0) and (stats[:, 3] == 0).all()
        delta = np.abs(1.0 - np.sqrt(stats[:, 0]))[:, None]
        assert delta.max() < 1e-6
        assert np.all(np.abs(vk - want_v) <= (delta + 2 * EPS32) * np.abs(want_v))
        # (two roundings of the sum: the reference's and the restatement's own)
        assert np.all(np.abs(xo - want_x) <= 2 * EPS32 * np.abs(want_x) + (delta + 4 * EPS32) * s * np.abs(want_v))
        assert np.array_equal(stats[:, 2], (want_v != 0).sum(1))
        if run == "sega":
            assert margin.min() >= 0.9e-4 and (stats[:, 2] < 0.4 * W.shape[1]).all()      # sigma = 1 keeps about a third of a Gaussian-like row
            std = np.array([float(torch.from_numpy(w).std()) for w in W])
            assert np.all(np.abs(stats[:, 1] - std) <= 1e-6 * std)                        # torch's fp32 std of the row against the two-sum formula
        assert [t for t in c["t"]] == [f["edit_t"]] * n                                   # the timestep, not the index


def test_new_symbols_are_exported():
    """the C entry points are declared and bound, the Python surface has the chain on every layer"""
    import inspect
    from diffusion_pullback_amd import PullbackUNet, engine, lib
    from diffusion_pullback_amd.edit import EditUncondDiffusion
    names = ("dpb_direction_step", "dpb_direction_step_scratch_bytes", "dpb_shift_stats", "dpb_inv_jac_chain", "dpb_inv_jac_chain_scratch_bytes")
    for n in names:
        assert n in lib.SYMBOLS, n
    L = lib.load()                                                # binds every declared symbol: a missing one raises
    assert L.dpb_abi_version() == 1
    assert L.dpb_direction_step_scratch_bytes(3, 4097) == 3 * 2 * 2 * 8 and L.dpb_direction_step_scratch_bytes(0, 5) == 0
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dpb.h")).read()
    for n in names:
        assert n + "(" in header, n
    assert callable(engine.direction_step) and callable(engine.shift_stats) and callable(engine.Engine.inv_jac_chain)
    sig = inspect.signature(PullbackUNet.inv_jac_chain).parameters
    for a in ("x", "t", "u", "dirs", "signs", "steps", "step_size", "sega_sigma", "encoder_hidden_states", "op", "block_idx", "return_vk",
              "final_shift", "check"):
        assert a in sig, a
    assert sig["return_vk"].default is False and sig["final_shift"].default is True and sig["sega_sigma"].default is None
    assert hasattr(EditUncondDiffusion, "_run_parallel_h_chains")


def test_host_side_refusals_need_no_gpu():
    """the engine-independent entry points validate their host arguments before anything is launched"""
    import ctypes as C
    from diffusion_pullback_amd import lib
    L = lib.load()
    f = (C.c_float * 2)(1.0, float("nan"))
    assert L.dpb_direction_step(8, 8, 8, None, f, 0.0, 2, 4, 8, 8, 1 << 20, None) != 0 and b"step[1]" in L.dpb_last_error()
    assert L.dpb_direction_step(8, 8, 8, None, f, 0.0, 1, 4, 8, 8, 0, None) != 0 and b"scratch" in L.dpb_last_error()
    assert L.dpb_direction_step(None, 8, 8, None, f, 0.0, 1, 4, 8, 8, 64, None) != 0 and b"null" in L.dpb_last_error()
    d = (C.c_int32 * 2)(0, 3)
    s = (C.c_float * 2)(1.0, 1.0)
    assert L.dpb_shift_stats(8, 8, 8, 3, d, s, 2, 4, 8, None) != 0 and b"dir[1]=3" in L.dpb_last_error()
    assert L.dpb_shift_stats(8, 8, 8, 0, d, s, 1, 4, 8, None) != 0 and b"nu=0" in L.dpb_last_error()


def _parse(*argv):
    from diffusion_pullback_amd.main import parse_args
    return parse_args(["--note", "n", *argv])


def test_edit_xt_flags_and_parser_errors(capsys):
    a = _parse()
    assert (a.edit_xt, a.use_sega_reg, a.sega_reg_sigma, a.x_edit_step_size) == ("parallel-x", False, 1.0, 0)
    ok = _parse("--edit_xt", "parallel-h", "--x_edit_step_size", "2.5", "--use_sega_reg", "True", "--sega_reg_sigma", "0.5", "--model_name", "CelebA_HQ_HF")
    assert (ok.edit_xt, ok.use_sega_reg, ok.sega_reg_sigma, ok.x_edit_step_size) == ("parallel-h", True, 0.5, 2.5)
    for argv in (("--edit_xt", "parallel-y"), ("--edit_xt", "default"),
                 ("--edit_xt", "parallel-h"), ("--edit_xt", "parallel-h", "--x_edit_step_size", "0"),
                 ("--edit_xt", "parallel-h", "--x_edit_step_size", "-1"),
                 ("--edit_xt", "parallel-h", "--x_edit_step_size", "1", "--model_name", "stable-diffusion-v1-5")):
        with pytest.raises(SystemExit):
            _parse(*argv)
    capsys.readouterr()
    # --edit_xt is a flag now: it is no longer reported among the ignored ones
    _parse("--edit_xt", "parallel-x")
    assert "ignoring" not in capsys.readouterr().out
    # parallel-h lifts the local_projection rule of the h-space bases, parallel-x keeps it
    job = ("--run_edit_global_frechet_mean_zt", "True", "--frechet_mean_space", "h", "--local_projection", "False")
    with pytest.raises(SystemExit):
        _parse(*job)
    assert _parse(*job, "--edit_xt", "parallel-h", "--x_edit_step_size", "1").local_projection is False


def test_default_edit_xt_leaves_the_parsed_arguments_unchanged():
    """apart from the three new attributes the namespace of a run is what it was: same keys, same values, with the flag given or not"""
    argv = ("--run_edit_global_hungarian_mean_zt", "True", "--hungarian_mean_space", "h", "--pca_rank", "3", "--model_name", "CelebA_HQ_HF",
            "--x_edit_step_size", "1.5")
    a, b = vars(_parse(*argv)), vars(_parse(*argv, "--edit_xt", "parallel-x"))
    assert a == b
    from diffusion_pullback_amd.main import _FLAGS
    new = {"edit_xt", "use_sega_reg", "sega_reg_sigma"}
    assert new <= set(a) and new <= {f[0] for f in _FLAGS}
    before = {f[0] for f in _FLAGS} - new | {"note", "memory_bound", "distance_space", "memory_bound_given", "h_t_values", "sample_idx_1_values"}
    assert set(a) - new == before
