"""The yardstick of the Hungarian-matched mean (tests/_hungarian_ref.py) held to what is known without it, and the command line of its job; no GPU.

  - planted sets: the restatement recovers the planted permutations and signs, for both distances, and converges in two sweeps;
  - scipy's optimum equals the brute force over all k! assignments for k <= 6;
  - under 'cosine' the objective sum |<y_i, xhat_{b, pi_b(i)}>| never decreases from sweep to sweep;
  - main.parse_args takes --run_edit_global_hungarian_mean_zt for an unconditional net and refuses a Stable Diffusion model, a bad space and
    space h without the local projection."""
import numpy as np
import pytest

import _hungarian_ref as R


@pytest.mark.parametrize("distance", R.DISTANCES)
@pytest.mark.parametrize("b,k,n,sigma", [(7, 17, 257, 0.5), (33, 50, 4099, 1.0), (5, 128, 513, 1.0)])
def test_restatement_recovers_the_planted_assignment(b, k, n, sigma, distance):
    a, y, perm, sign = R.planted_set(np.random.default_rng(100 * k + b), b, k, n, sigma)
    Y, info = R.hungarian_mean_ref(a, distance=distance)
    assert (info["perm"] == perm).all() and (info["sign"] == sign).all()
    assert info["converged"] and info["sweeps"] == 2 and info["changed"] == [b * k, 0]
    assert (info["perm"][0] == np.arange(k)).all() and (info["sign"][0] == 1).all()
    # the mean is the planted frame in member 0's order and signs, up to the noise left after averaging B members (sigma / sqrt(B) per row)
    held = np.argmax(np.abs(R.overlaps(R.unit_rows(a[:1]), y))[0], axis=0)          # the planted direction row i of member 0 holds
    cos = np.abs(np.sum(R.unit_rows(Y) * y[held], axis=1))
    assert cos.min() > 1.0 / np.sqrt(1.0 + 2.0 * sigma ** 2 / b)
    assert np.allclose(np.linalg.norm(Y.astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert (info["weight"] > 0).all() and (info["weight"] <= 1 + 1e-12).all()


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6])
def test_scipy_optimum_is_the_brute_force_optimum(k):
    rng = np.random.default_rng(k)
    for trial in range(8):
        d = rng.uniform(size=(k, k)) if trial % 2 else rng.integers(0, 4, size=(k, k)).astype(np.float64)
        col, total = R.assign(d)
        assert sorted(col.tolist()) == list(range(k))
        assert abs(total - R.brute_force(d)) <= 1e-14 * k


@pytest.mark.parametrize("b,k,n", [(7, 17, 257), (5, 64, 300)])
def test_cosine_objective_never_decreases(b, k, n):
    """Given the anchor, the assignment and the signs maximise sum_i <y_i, S_i> with S_i = sum_b sigma x; y_i = S_i / |S_i| maximises it over unit rows;
    and |c| >= sigma c under the next assignment.  The only loss is the rounding of Y to float32: 2^-24 relative per overlap, B k overlaps of
    at most 1."""
    a = R.gaussian_set(np.random.default_rng(b + k), b, k, n)
    _, info = R.hungarian_mean_ref(a, distance="cosine", max_sweeps=20)
    obj = np.array(info["objective"])
    assert info["converged"] and info["sweeps"] >= 2
    assert (np.diff(obj) >= -b * k * 2.0 ** -24).all(), obj


def test_one_basis_is_its_own_mean():
    a = R.gaussian_set(np.random.default_rng(3), 1, 9, 40)
    Y, info = R.hungarian_mean_ref(a)
    assert (info["perm"][0] == np.arange(9)).all() and (info["sign"] == 1).all() and info["sweeps"] == 2
    assert np.abs(Y - R.unit_rows(a[0])).max() <= 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------ the command line
BASE = ["--note", "t", "--dataset_name", "Random", "--run_edit_global_hungarian_mean_zt", "True"]


def _parse(argv):
    from diffusion_pullback_amd import main as m
    return m.parse_args(argv)


def test_cli_takes_the_flags_for_an_unconditional_net():
    args = _parse(BASE + ["--model_name", "CelebA_HQ_HF"])
    assert args.run_edit_global_hungarian_mean_zt is True
    assert args.hungarian_mean_space == "x" and args.hungarian_distance == "1/cosine" and args.hungarian_max_sweeps == 20
    args = _parse(BASE + ["--model_name", "CelebA_HQ_HF", "--hungarian_mean_space", "h", "--hungarian_distance", "cosine", "--hungarian_max_sweeps", "3"])
    assert (args.hungarian_mean_space, args.hungarian_distance, args.hungarian_max_sweeps) == ("h", "cosine", 3)
    assert _parse(["--note", "t", "--model_name", "CelebA_HQ_HF"]).run_edit_global_hungarian_mean_zt is False


@pytest.mark.parametrize("extra,word", [
    (["--model_name", "stable-diffusion-v1-5"], "unconditional"),
    (["--model_name", "CelebA_HQ_HF", "--hungarian_mean_space", "z"], "hungarian_mean_space"),
    (["--model_name", "CelebA_HQ_HF", "--hungarian_mean_space", "h", "--local_projection", "False"], "local_projection"),
    (["--model_name", "CelebA_HQ_HF", "--hungarian_distance", "euclid"], "hungarian_distance"),
])
def test_cli_error_rules(extra, word, capsys):
    with pytest.raises(SystemExit):
        _parse(BASE + extra)
    assert word in capsys.readouterr().err
