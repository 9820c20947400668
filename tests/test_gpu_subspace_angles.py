"""dpb_cross_gram / dpb_subspace_angles / geometry.py / run_tangent_space_distance on the GPU.

Reference: scipy.linalg.subspace_angles in float64 on the same fp32 inputs.  Bar: 1e-6 rad per angle, dist within 1e-6 relative (tests/_angles_ref.py
re-measures on the CPU what the method itself yields: a few 1e-8).  Where every angle of a pair is zero by construction -- (k, N) = (1, 7) and
(4, 4) -- the reference distance is itself only rounding noise of ~1e-8 and a relative bar on it measures nothing: there dist is held to the per-angle
bar, |dist - dist_scipy| <= 1e-6 sqrt(k).  The exact-Gram cases use small integers, for which the fp64 result has no rounding at all.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

from _angles_ref import BAR, SHAPES_GPU, VARIANTS, crafted, scipy_angles

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _geo():
    from diffusion_pullback_amd import geometry
    return geometry


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(k, N, variant):
    A, B = crafted(k, N, variant)
    return A, B, scipy_angles(A, B)


def _check_pair(theta, dist, want, k, what):
    theta, dist = np.asarray(theta, dtype=np.float64), float(dist)
    err = np.abs(theta - want).max()
    dref = np.linalg.norm(want)
    print(f"{what}: worst |theta - scipy| = {err:.2e} rad, dist {dist:.9g} vs {dref:.9g}")
    assert err <= BAR, what
    assert (np.diff(theta) <= 0).all(), what
    if dref > 1e-3:
        assert abs(dist - dref) <= BAR * dref, what
    else:                                         # every angle is zero by construction (module docstring)
        assert abs(dist - dref) <= BAR * np.sqrt(k), what
    assert abs(dist - np.linalg.norm(theta)) <= 2.0 ** -22 * max(np.linalg.norm(theta), 1e-30), what      # dist = ||theta||_2 (fp32 roundings of theta and dist)


# ------------------------------------------------------------------------------------------------------------ exact Gram
@pytest.mark.parametrize("Ra,Rb,N", [(37, 21, 1003), (16, 16, 4), (1, 1, 1), (130, None, 4099), (16, 5, 70001)])
def test_cross_gram_is_exact_on_small_integers(Ra, Rb, N):
    """entries in {-3..3}: every product and every partial sum is an integer below 2^53, so fp64 holds G exactly -- a swapped row map of the f64 MFMA,
    a missed tail of rows or of N, an un-summed slice or a wrong mirror shows as a wrong integer.  X and Y are unrelated (asymmetric)."""
    rng = np.random.default_rng(Ra * 1000 + N)
    X = rng.integers(-3, 4, size=(Ra, N)).astype(np.float32)
    Y = None if Rb is None else rng.integers(-3, 4, size=(Rb, N)).astype(np.float32)
    G = _geo().cross_gram(_dev(X), None if Y is None else _dev(Y))
    want = X.astype(np.int64) @ (X if Y is None else Y).astype(np.int64).T
    assert G.dtype == torch.float64 and tuple(G.shape) == want.shape
    assert np.array_equal(G.cpu().numpy(), want.astype(np.float64))
    G2 = _geo().cross_gram(_dev(X), None if Y is None else _dev(Y))
    assert torch.equal(G, G2)


def test_cross_gram_on_reals_is_fp64_accurate_and_symmetric():
    """N % 4 != 0 and a misaligned view: the scalar load path; fp64 accumulation of exact products -- error ~1e-16 of sum |x y|, where an fp32
    accumulation would leave ~1e-7"""
    rng = np.random.default_rng(3)
    X = rng.standard_normal((70, 2051)).astype(np.float32)
    buf = torch.zeros(70 * 2051 + 1, dtype=torch.float32, device=DEV)
    Xd = buf[1:].view(70, 2051)                   # 4-byte aligned only
    Xd.copy_(_dev(X))
    G = _geo().cross_gram(Xd).cpu().numpy()
    X64 = X.astype(np.float64)
    assert np.array_equal(G, G.T)
    assert np.abs(G - X64 @ X64.T).max() <= 1e-13 * (np.abs(X64) @ np.abs(X64).T).max()
    assert np.array_equal(G, _geo().cross_gram(_dev(X)).cpu().numpy())        # the 16-byte path adds in the same order
    assert np.array_equal(G[:33, 40:], _geo().cross_gram(_dev(X[:33]), _dev(X[40:])).cpu().numpy())      # an entry does not depend on Ra, Rb, position


# ------------------------------------------------------------------------------------------------------------ angles
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("k,N", SHAPES_GPU)
def test_angles_meet_scipy_at_the_bar(k, N, variant):
    A, B, want = _case(k, N, variant)
    g = _geo()
    theta, dist = g.subspace_angles_and_distance(_dev(A), _dev(B))
    assert tuple(theta.shape) == (1, 1, k) and tuple(dist.shape) == (1, 1) and theta.dtype == torch.float32
    _check_pair(theta[0, 0].cpu().numpy(), dist[0, 0].cpu(), want, k, f"k={k} N={N} {variant}")
    if (k, N) == (4, 4):                          # both spans are the whole space
        assert float(theta.max()) <= BAR
    # self mode over the two bases: exactly symmetric, an exactly zero diagonal, the same pair
    ts, ds = g.subspace_angles_and_distance(torch.stack([_dev(A), _dev(B)]))
    assert torch.equal(ts[0, 1], theta[0, 0]) and torch.equal(ts[1, 0], ts[0, 1]) and torch.equal(ds, ds.t()) and torch.equal(ds[0, 1], dist[0, 0])
    assert (ts[0, 0] == 0).all() and (ts[1, 1] == 0).all() and ds[0, 0] == 0 and ds[1, 1] == 0
    assert torch.equal(g.subspace_angles(_dev(A), _dev(B)), theta) and torch.equal(g.geodesic_distance(_dev(A), _dev(B)), dist)


def test_python_argument_checks():
    g = _geo()
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(ValueError, match="128"):
        g.subspace_angles(z(1, 129, 256))
    with pytest.raises(ValueError, match="N = 4"):
        g.subspace_angles(z(1, 5, 4))
    with pytest.raises(ValueError, match="must match"):
        g.subspace_angles(z(2, 3, 16), z(2, 4, 16))
    with pytest.raises(ValueError, match="must match"):
        g.subspace_angles(z(2, 3, 16), z(2, 3, 17))
    A, B, want = _case(5, 4096, "mixed")          # any float dtype is converted
    th = g.subspace_angles(_dev(A).double(), _dev(B).double())
    assert th.dtype == torch.float32 and np.abs(th[0, 0].cpu().numpy() - want).max() <= BAR


# ------------------------------------------------------------------------------------------------------------ batch invariance
def test_batch_invariance_is_bitwise():
    k, N = 17, 3001
    rng = np.random.default_rng(17)
    A = _dev(rng.standard_normal((7, k, N)).astype(np.float32))
    B = _dev((0.7 * A[:5].cpu().numpy() + 0.3 * rng.standard_normal((5, k, N))).astype(np.float32))      # related spans: angles of every size
    g = _geo()
    theta, dist = g.subspace_angles_and_distance(A, B)
    assert torch.isfinite(theta).all()
    t2, d2 = g.subspace_angles_and_distance(A, B)
    assert torch.equal(theta, t2) and torch.equal(dist, d2)                                             # two runs
    for i in range(7):
        for j in range(5):
            t1, d1 = g.subspace_angles_and_distance(A[i], B[j])                                         # the pair's own call
            assert torch.equal(t1[0, 0], theta[i, j]) and torch.equal(d1[0, 0], dist[i, j]), (i, j)
    ts, ds = g.subspace_angles_and_distance(torch.cat([A, B]))                                          # self mode over the concatenation
    assert torch.equal(ts[:7, 7:], theta) and torch.equal(ds[:7, 7:], dist)
    assert torch.equal(ts, ts.transpose(0, 1)) and torch.equal(ds, ds.t())
    one = int(g.L.load().dpb_subspace_angles_scratch_bytes(1, 1, k, N))
    for cap in (one, int(g.L.load().dpb_subspace_angles_scratch_bytes(3, 3, k, N))):                    # blocks of 1 and of 3 bases
        tb, db = g.subspace_angles_and_distance(A, B, max_bytes=cap)
        assert torch.equal(tb, theta) and torch.equal(db, dist)
        tb, db = g.subspace_angles_and_distance(torch.cat([A, B]), None, max_bytes=cap)
        assert torch.equal(tb, ts) and torch.equal(db, ds)
    assert torch.equal(g.subspace_angles(A, B, max_bytes=one), theta)


# ------------------------------------------------------------------------------------------------------------ degenerate bases
def test_degenerate_bases_give_nan_rows_and_columns_only():
    k, N = 6, 515
    rng = np.random.default_rng(9)
    A = rng.standard_normal((4, k, N)).astype(np.float32)
    A[1, 2] = 0.0                                 # a zero row
    A[3, 4] = A[3, 1]                             # a duplicated row
    g = _geo()
    theta, dist = g.subspace_angles_and_distance(_dev(A), check=False)
    theta, dist = theta.cpu().numpy(), dist.cpu().numpy()
    for i in range(4):
        for j in range(4):
            if i in (1, 3) or j in (1, 3):
                assert np.isnan(theta[i, j]).all() and np.isnan(dist[i, j]), (i, j)
            elif i == j:
                assert (theta[i, j] == 0).all() and dist[i, j] == 0
            else:
                _check_pair(theta[i, j], dist[i, j], scipy_angles(A[i], A[j]), k, f"pair {i},{j}")
    with pytest.raises(ValueError, match=r"indices \[1, 3\]"):
        g.subspace_angles(_dev(A))
    with pytest.raises(ValueError, match=r"indices \[1, 3\]"):
        g.geodesic_distance(_dev(A))
    tc, dc = g.subspace_angles_and_distance(_dev(A[[0, 2]]), _dev(A), check=False)                      # cross mode: columns 1 and 3 only
    assert torch.isnan(dc[:, [1, 3]]).all() and torch.isfinite(dc[:, [0, 2]]).all() and torch.isnan(tc[:, [1, 3]]).all()
    with pytest.raises(ValueError, match=r"indices \[\] of A, \[1, 3\] of B"):
        g.subspace_angles(_dev(A[[0, 2]]), _dev(A))


# ------------------------------------------------------------------------------------------------------------ the job, end to end
def _argv(tmp, kind, *more):
    common = ["--note", "t", "--result_folder", str(tmp), "--device", DEV, "--net_scale", "small", "--pca_rank", "4", "--num_local_basis", "3",
              "--h_t_list", "0.8,0.5", "--dataset_name", "Random", *more]
    if kind == "sd":
        return common + ["--model_name", "runwayml/stable-diffusion-v1-5", "--edit_prompt", "tiger", "--for_steps", "20", "--inv_steps", "20"]
    return common + ["--model_name", "CelebA_HQ_HF", "--performance_boosting_t", "0.2"]


@pytest.mark.parametrize("kind", ["sd", "ddpm"])
def test_distance_job_end_to_end(tmp_path, kind, monkeypatch):
    """the toy nets of tests/test_gpu_tspace.py: sample 3 bases x 2 timesteps at pca_rank 4 through the CLI entry, then the distance job for both
    spaces; the saved dist against scipy on the saved files, names and order against the sampling job's; a deleted file makes the job raise"""
    from diffusion_pullback_amd import main as m
    root = os.path.join(str(tmp_path), "inputs")
    real_preset = m.preset

    def preset(args):                             # the drivers' basis cache goes under the test's directory
        args = real_preset(args)
        args.input_root = root
        return args
    monkeypatch.setattr(m, "preset", preset)
    m.main(_argv(tmp_path, kind, "--run_sample_encoder_local_tangent_space_zt", "True"))
    if kind == "sd":
        d = os.path.join(root, "local_encoder_pullback_stable_diffusion-dataset_Random-num_steps_20-pca_rank_4")
        name = lambda i, ht: f'zt-Random_{i}-{ht}T-"tiger"-mid-block_0-seed_0'
    else:
        d = os.path.join(root, "local_encoder_pullback_uncond-model_CelebA_HQ_HF-dataset_Random-num_steps_100-pca_rank_4")
        name = lambda i, ht: f"xt-Random_{i}-{ht}T-mid-block_0-seed_0"
    order = [(i, ht) for ht in (0.8, 0.5) for i in range(3)]
    for space, pre in (("x", "vT-"), ("h", "u-")):
        ed = m.main(_argv(tmp_path, kind, "--run_tangent_space_distance", "True", "--distance_space", space))
        out_path = os.path.join(d, ed.EXP_NAME + ".pt")
        assert os.path.basename(out_path).startswith(f"tangent_space_distance-{space}-") and os.path.exists(out_path)
        assert os.path.exists(out_path[:-3] + ".png")
        out = torch.load(out_path)
        assert out["names"] == [name(i, ht) for i, ht in order] and out["idx"] == [i for i, _ in order] and out["h_t"] == [ht for _, ht in order]
        assert tuple(out["theta"].shape) == (6, 6, 4) and tuple(out["dist"].shape) == (6, 6)
        bases = [torch.load(os.path.join(d, pre + n + ".pt"), map_location="cpu").float().numpy() for n in out["names"]]
        bases = [b if space == "x" else b.T for b in bases]
        for i in range(6):
            assert out["dist"][i, i] == 0
            for j in range(i + 1, 6):
                _check_pair(out["theta"][i, j].numpy(), out["dist"][i, j], scipy_angles(bases[i], bases[j]), 4, f"{kind} {space} pair {i},{j}")
                assert torch.equal(out["theta"][i, j], out["theta"][j, i])
    os.remove(os.path.join(d, "vT-" + name(2, 0.5) + ".pt"))
    with pytest.raises(ValueError, match=re.escape("vT-" + name(2, 0.5) + ".pt")):
        m.main(_argv(tmp_path, kind, "--run_tangent_space_distance", "True", "--distance_space", "x"))
