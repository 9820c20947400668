"""geometry.linear_assignment (dpb_linear_assignment, csrc/hungarian.hip) on the GPU against scipy.optimize.linear_sum_assignment on the identical
float64 matrices.

Bars.  Every output row is a permutation.  Uniform-random costs: the two totals are sums of k float64 terms of the same kind, so they agree within
k 2^-52 max|cost| 4.  Small-integer costs with many ties: the sums are exact, so the totals are EQUAL (the permutations may differ: several are
optimal).  The device's total is also held to the sum of its own permutation's entries."""
import functools

import numpy as np
import pytest
import torch

import _hungarian_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KS = [1, 2, 3, 17, 50, 64, 65, 128]
BS = [1, 7, 33]


def _solve(cost):
    from diffusion_pullback_amd import geometry
    col, total = geometry.linear_assignment(torch.tensor(np.asarray(cost), device=DEV))
    return col.cpu().numpy(), total.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _uniform(b, k):
    d = np.random.default_rng(1000 * k + b).uniform(size=(b, k, k))
    d.setflags(write=False)
    return d, np.array([R.assign(m)[1] for m in d])


@functools.lru_cache(maxsize=None)
def _integers(b, k):
    d = np.random.default_rng(2000 * k + b).integers(0, 4, size=(b, k, k)).astype(np.float64)
    d.setflags(write=False)
    return d, np.array([R.assign(m)[1] for m in d])


def _check_perms(col, d):
    b, k, _ = d.shape
    assert col.shape == (b, k) and col.dtype == np.int32
    assert (np.sort(col, axis=1) == np.arange(k)).all()
    return np.array([d[i][np.arange(k), col[i]].sum() for i in range(b)])


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("k", KS)
def test_uniform_costs_reach_scipys_optimum(k, B):
    d, want = _uniform(B, k)
    col, total = _solve(d)
    own = _check_perms(col, d)
    bar = k * 2.0 ** -52 * np.abs(d).max() * 4
    print(f"k = {k}, B = {B}: total against scipy {np.abs(total - want).max():.2e}, against its own permutation {np.abs(total - own).max():.2e} (bar {bar:.2e})")
    assert np.abs(total - want).max() <= bar
    assert np.abs(total - own).max() <= bar


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("k", KS)
def test_integer_costs_with_ties_give_equal_totals(k, B):
    d, want = _integers(B, k)
    col, total = _solve(d)
    own = _check_perms(col, d)
    assert (total == want).all() and (total == own).all()


@pytest.mark.parametrize("k", [2, 3, 17, 64, 65, 128])
def test_product_matrix_needs_the_reversed_pairing(k):
    """cost[i][j] = (i + 1)(j + 1): by the rearrangement inequality the minimum pairs the largest row with the smallest column, uniquely; the greedy
    row minimum would give row 0 column 0"""
    i = np.arange(1, k + 1, dtype=np.float64)
    col, total = _solve(np.outer(i, i)[None])
    assert (col[0] == np.arange(k)[::-1]).all()
    assert total[0] == float((i * i[::-1]).sum())


@pytest.mark.parametrize("k", [1, 5, 64, 100])
def test_special_matrices(k):
    rng = np.random.default_rng(k)
    flat = np.full((k, k), 2.5)
    p = rng.permutation(k)
    dominant = rng.uniform(1.0, 2.0, size=(k, k))
    dominant[np.arange(k), p] = rng.uniform(0.0, 0.01, size=k)             # that pairing costs < 0.01 k <= 1; any other holds two entries >= 1
    mixed = rng.uniform(size=(k, k))
    mixed[rng.uniform(size=(k, k)) < 0.5] = 2.0 ** 40                       # entries of 2^40 among O(1) ...
    mixed[np.arange(k), p] = rng.uniform(size=k)                            # ... and a pairing that avoids them
    d = np.stack([flat, dominant, mixed])
    col, total = _solve(d)
    own = _check_perms(col, d)
    want = np.array([R.assign(m)[1] for m in d])
    assert total[0] == 2.5 * k and (col[0] == np.arange(k)).all()           # all ties: the lowest column index wins every step
    assert (col[1] == p).all()
    bar = k * 2.0 ** -52 * np.abs(d).max(axis=(1, 2)) * 4                   # (the duals of the third matrix carry 2^40: the bar's max|cost|)
    print(f"k = {k}: totals against scipy {np.abs(total - want)}, bars {bar}")
    assert (np.abs(total - want) <= bar).all() and (np.abs(total - own) <= bar).all()
    assert total[2] < 2.0 ** 40


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("k", [3, 65])
def test_a_non_finite_entry_spoils_only_its_own_problem(k, bad):
    d = np.random.default_rng(k).uniform(size=(5, k, k))
    d[2, k // 2, k - 1] = bad
    col, total = _solve(d)
    assert (col[2] == -1).all() and np.isnan(total[2])
    keep = [0, 1, 3, 4]
    clean_col, clean_total = _solve(d[keep])
    assert (col[keep] == clean_col).all() and (total[keep] == clean_total).all()
    _check_perms(col[keep], d[keep])


@pytest.mark.parametrize("k", [17, 64, 128])
def test_batch_invariant_and_reproducible(k):
    d, _ = _uniform(33, k)
    col, total = _solve(d)
    col2, total2 = _solve(d)
    assert (col == col2).all() and (total == total2).all()
    for b in (0, 5, 32):
        c1, t1 = _solve(d[b:b + 1])
        assert (c1[0] == col[b]).all() and t1[0] == total[b]
    ti, _ = _integers(33, k)                                                 # with ties the choice among optima must not depend on the batch either
    col, total = _solve(ti)
    for b in (0, 32):
        c1, t1 = _solve(ti[b:b + 1])
        assert (c1[0] == col[b]).all() and t1[0] == total[b]


def test_bad_arguments():
    from diffusion_pullback_amd import geometry
    with pytest.raises(ValueError):
        geometry.linear_assignment(torch.zeros(2, 129, 129, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        geometry.linear_assignment(torch.zeros(2, 3, 4, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        geometry.linear_assignment(torch.zeros(2, 3, 3, dtype=torch.float32, device=DEV))
