"""CPU half of the dpb_orth pins (tests/test_gpu_orth.py): the float64 restatement of the method (tests/_orth_ref.py) must meet every bound the GPU
tests hold the kernels to, on every accuracy case; each float32 mutant must miss the vec bound 16-fold -- the standing proof that the bars have
teeth; the input conditions the bars rest on are asserted, so a seed change cannot silently void a check; and the exact cases' closed forms are
checked against the restatement.  Non-finite input: the restatement meets the rule of include/dpb.h on every case the GPU tests run, through the same
two assertions, and the three traits the kernels had before the rule are kept as mutants that fail them."""
import numpy as np
import pytest

import _orth_ref as R

IDS = lambda c: f"{c[0]}x{c[1]}-{c[2]}dec-{c[3]}"


@pytest.mark.parametrize("case", R.ACCURACY_CASES, ids=IDS)
def test_restatement_meets_every_gpu_bound(case):
    k, N, decades, route = case
    c = R.case(k, N, decades)
    R.check(*R.restate(c.W, c.Vprev), c, k, N, decades, route)


@pytest.mark.parametrize("case", R.ACCURACY_CASES, ids=IDS)
def test_input_conditions_of_every_accuracy_case(case):
    """no case is skipped or exempted: every row of every case has an overlap with Vprev that rounding cannot flip, every adjacent pair of singular
    values a gap that keeps single vectors well defined, and the spectrum is the one asked for"""
    k, N, decades, _ = case
    c = R.case(k, N, decades)
    ov, gap = R.input_conditions(c.W, c.Vprev, c.V_ref, c.sqrtS)
    print(f"k={k} N={N} decades={decades}: min overlap {ov:.2e}, min gap {gap:.2e}")
    assert len(c.V_ref) == k and len(c.floor_vec) == k            # the share of rows left out is zero
    assert ov >= R.MIN_OVERLAP
    assert gap >= R.MIN_GAP
    assert np.allclose(c.sqrtS ** 2, np.logspace(0.0, -float(decades), k), rtol=1e-5)
    assert (c.floor_vec > 0).all() and c.floor_on > 0


@pytest.mark.parametrize("k,N", R.MUTANT_CASES)
@pytest.mark.parametrize("mutant", ["gram_fp32", "apply_fp32"])
def test_fp32_mutants_miss_the_vec_bound(k, N, mutant):
    """one case per k band of the apply kernels (k <= 16, 17 .. 56, > 56)"""
    c = R.case(k, N, 2)
    kw = dict(gram_dtype=np.float32) if mutant == "gram_fp32" else dict(apply_dtype=np.float32)
    m = R.measure(*R.restate(c.W, c.Vprev, **kw), c)
    print(f"k={k} N={N} {mutant}: vec {m['vec']:.1f} on {m['on']:.1f} s_ulps {m['s_ulps']:.2f}")
    assert m["vec"] >= R.MUTANT_FACTOR * R.bounds(2)[0]
    with pytest.raises(AssertionError):
        R.check(*R.restate(c.W, c.Vprev, **kw), c, k, N, 2, mutant)


def test_mutant_cases_cover_the_three_bands():
    ks = [k for k, _ in R.MUTANT_CASES]
    assert any(k <= 16 for k in ks) and any(16 < k <= 56 for k in ks) and any(k > 56 for k in ks)
    assert all((k, N, 2) in {(a, b, d) for a, b, d, _ in R.ACCURACY_CASES} for k, N in R.MUTANT_CASES)


@pytest.mark.parametrize("decades", R.BEYOND)
def test_beyond_the_pinned_domain_the_method_itself_degrades(decades):
    """five and six decades: eps64 cond^2 exceeds the fp32 floor -- the float64 restatement leaves the vec bound, which is why the domain ends at
    four decades; the leading half of s stays exact"""
    k, N = R.LADDER_SHAPE
    c = R.case(k, N, decades)
    V, s, conv = R.restate(c.W, c.Vprev)
    m = R.measure(V, s, conv, c)
    print(R.line(k, N, decades, "beyond", m))
    assert np.isfinite(V).all() and m["s_ulps_rows"][:k // 2].max() <= 1.0
    assert m["vec"] > R.bounds(4)[0]


@pytest.mark.parametrize("k,N", R.CONVERGED)
def test_restatement_on_converged_input(k, N):
    c = R.converged_case(k, N)
    ov, gap = R.input_conditions(c.W, c.Vprev, c.V_ref, c.sqrtS)
    assert ov >= 0.99 and gap >= R.MIN_GAP
    m = R.check(*R.restate(c.W, c.Vprev), c, k, N, 2, "converged")
    assert m["dmax"] <= 1e-6                     # the fixed point: V is Vprev up to its own departure from orthonormality


# ------------------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("k", R.EXACT_K)
def test_ties_closed_form(k):
    W, V_want, s_want, Vp = R.make_ties(k, 300)
    sig = W.max(axis=1)
    assert sorted(set(sig)) == [1.0, 2.0, 4.0] and (np.diff(sig) != 0).any() and not (np.diff(sig) <= 0).all()      # tie groups, shuffled
    assert ((W != 0).sum(axis=1) == 1).all() and ((W != 0).sum(axis=0) <= 1).all()                                 # one-hot, distinct columns
    V, s, conv = R.restate(W, Vp)
    assert np.array_equal(V, V_want) and np.array_equal(s, s_want) and np.array_equal(conv, [0.0, 0.0])
    # the expected order, stated independently: descending sigma, ties in input order
    cols = W.argmax(axis=1)
    order = sorted(range(k), key=lambda i: (-sig[i], i))
    assert np.array_equal(V_want.argmax(axis=1), cols[order]) and np.array_equal(s_want, np.sqrt(sig[order]).astype(np.float32))


@pytest.mark.parametrize("k", R.EXACT_K)
def test_dead_direction_closed_form(k):
    c = R.dead_case(k, 700)
    assert not c.W_full[k // 2].any() and np.array_equal(np.delete(c.W_full, k // 2, axis=0), c.W)
    ov, gap = R.input_conditions(c.W, c.Vprev, c.V_ref, c.sqrtS)
    assert ov >= R.MIN_OVERLAP and gap >= R.MIN_GAP
    V, s, conv = R.restate(c.W_full, c.Vprev_full)
    assert not V[-1].any() and s[-1] == 0
    R.check(V, s, conv, c, k, 700, 2, "dead", Vprev=c.Vprev_full)


@pytest.mark.parametrize("k", R.EXACT_K)
def test_all_zero_closed_form(k):
    _, Vp = R.make(k, 700, 2)
    V, s, conv = R.restate(np.zeros_like(Vp), Vp)
    assert not V.any() and not s.any()
    want = np.linalg.norm(Vp.astype(np.float64))
    assert abs(conv[0] - want) <= R.U32 * want and conv[1] == np.abs(Vp).max()


@pytest.mark.parametrize("k,N", R.DEFICIENT)
def test_restatement_near_rank_deficiency(k, N):
    """two rows are fp32 combinations of the others: the two trailing singular values are rounding noise (~1e-8 of the leading ones) and so are their
    vectors; the leading k - 2 keep the bounds"""
    c = R.deficient_case(k, N)
    assert len(c.V_ref) == k - 2
    full = np.linalg.svd(c.W.astype(np.float64), compute_uv=False)
    assert full[-2] <= 1e-6 * full[0] and full[k - 3] >= 1e-3 * full[0]
    ov, gap = R.input_conditions(c.W, c.Vprev, c.V_ref, c.sqrtS)
    assert ov >= R.MIN_OVERLAP and gap >= R.MIN_GAP
    V, s, conv = R.restate(c.W, c.Vprev)
    assert np.isfinite(V).all() and np.isfinite(s).all() and (s >= 0).all()
    R.check(V, s, conv, c, k, N, 2, "deficient")


# ------------------------------------------------------------------------------------------------------------ non-finite input (include/dpb.h)
@pytest.mark.parametrize("how", R.NF_POISONS)
@pytest.mark.parametrize("k,N", R.NF_SHAPES)
def test_restatement_non_finite_w_is_all_nan(k, N, how):
    """every case of tests/test_gpu_orth.py::test_non_finite_w_is_all_nan_and_leaves_no_state, same assertion"""
    W, Vp = R.inputs(k, N, 2)
    Wb = R.poisoned(W, how)
    assert (~np.isfinite(Wb)).sum() == (N if how == "nan-row" else 1)
    R.assert_all_nan(*R.restate(Wb, Vp), f"k={k} N={N} {how}")


@pytest.mark.parametrize("how", [h for h in R.NF_POISONS if h != "nan-row"])
@pytest.mark.parametrize("k", R.NF_VPREV_K)
def test_restatement_non_finite_vprev_only(k, how):
    W, Vp = R.inputs(k, R.NF_N, 2)
    R.assert_vprev_rule(R.restate(W, R.poisoned(Vp, how)), R.restate(W, Vp), f"k={k} Vprev {how}")


@pytest.mark.parametrize("mutant,symptom", [("rank_plain", "s"), ("clamp", "s"), ("fmax", "conv")])
@pytest.mark.parametrize("k", [5, 17, 128])
def test_non_finite_mutants_fail_the_gpu_assertions(k, mutant, symptom):
    """the method without the Gram-diagonal detection and with ONE of the three traits it had: each fails assert_all_nan, the assertion of the GPU
    tests, in its own way -- the plain ranking leaves slots of `order` unwritten (not a permutation) and s comes back finite through them, the
    lam > 0 ? lam : 0 clamp returns s == 0 beside a NaN V, the NaN-dropping maximum returns conv[1] == 0 beside a NaN V"""
    W, Vp = R.inputs(k, R.NF_N, 2)
    Wb = R.poisoned(W, "nan-first")
    V, s, conv = R.restate(Wb, Vp, mutant=mutant)
    print(f"k={k} {mutant}: s[:3] {s[:3]} conv {conv} NaN in V {int(np.isnan(V).sum())} / {V.size}")
    with pytest.raises(AssertionError) as err:
        R.assert_all_nan(V, s, conv, mutant)
    assert f"'{symptom}'" in str(err.value), str(err.value)[:200]
    lam = np.full(k, np.nan)
    if mutant == "rank_plain":
        order = R.rank_scatter(lam, total=False)
        assert sorted(order) != list(range(k)) and (order == R.POISON).sum() == k - 1 and np.isfinite(s[1:]).all()
    elif mutant == "clamp":
        assert not s.any() and np.isnan(V).all()
    else:
        assert conv[1] == 0 and np.isnan(conv[0]) and np.isnan(V).all()
    assert sorted(R.rank_scatter(lam)) == list(range(k))         # and the total order scatters a permutation: index order among NaNs
    assert list(R.rank_scatter(lam)) == list(range(k))


def test_rank_scatter_is_the_stable_descending_order_on_numbers_and_nan_first():
    rng = np.random.default_rng(11)
    for k in (1, 2, 5, 16, 33):
        lam = rng.integers(0, 4, k).astype(np.float64)           # ties
        assert list(R.rank_scatter(lam)) == list(np.argsort(-lam, kind="stable")) == list(R.rank_scatter(lam, total=False))
        lam[rng.integers(0, k)] = np.nan
        order = R.rank_scatter(lam)
        assert sorted(order) == list(range(k)) and np.isnan(lam[order[0]])
        rest = lam[order[1:]]
        assert (np.diff(rest) <= 0).all()


def test_max_nan_keeps_what_python_max_drops():
    assert np.isnan(R.max_nan(np.float32(0), np.float32(np.nan))) and max(np.float32(0), np.float32(np.nan)) == 0
    assert R.max_nan(np.float32(0), np.float32(2)) == 2


# ------------------------------------------------------------------------------------------------------------ the measures themselves
def test_measures_read_one_on_the_rounded_reference_and_see_a_small_slip():
    k, N = 16, 4099
    c = R.case(k, N, 2)
    Vi = c.V_ref.astype(np.float32)
    c0, c1, _ = R.conv_recomputed(Vi, c.Vprev)
    m = R.measure(Vi, c.sqrtS.astype(np.float32), np.array([c0, c1], dtype=np.float32), c)
    assert m["vec"] == 1.0 and m["on"] == 1.0 and m["s_ulps"] <= 0.5 and m["conv0_ulps"] <= 0.5 and m["conv1_err"] <= R.U32 * m["dmax"] / 2
    bad = Vi.copy()
    bad[3] += np.float32(3e-7) * Vi[4]            # a tilt of 3e-7 rad: invisible to a |cos| > 1 - 1e-5 bar (cos = 1 - 4.5e-14)
    assert R.measure(bad, c.sqrtS, [c0, c1], c)["vec"] > 4.0
    assert R.measure(Vi, c.sqrtS * (1 + 3e-7), [c0, c1], c)["s_ulps"] > 2.0
    assert R.measure(Vi, c.sqrtS, [c0 * (1 + 3e-7), c1], c)["conv0_ulps"] > 2.0
