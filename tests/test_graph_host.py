"""CPU checks of tests/_graph_ref.py: the generator is deterministic, the fixed corpus reaches every bookkeeping feature and motif, the exact tier's
precondition holds for every seed and pass, its adjoint identity holds as integers, the real tier's autograd agrees with central finite differences,
and no dropped bookkeeping contribution is invisible to the corpus."""
import pytest
import torch

import _graph_ref as R
from _graph_ref import BF, F16, F32

CORPUS = [("exact", s) for s in R.EXACT_SEEDS] + [("real", s) for s in R.REAL_SEEDS]
IDS = [f"{t}{s}" for t, s in CORPUS]


@pytest.mark.parametrize("tier,seed", CORPUS, ids=IDS)
def test_generator_is_deterministic(tier, seed):
    a, b = R.random_tape(seed, tier), R.random_tape(seed, tier)
    assert list(a) == list(b) and a.meta == b.meta and (a.B, a.kps, a.attempt) == (b.B, b.kps, b.attempt)
    assert a.params.keys() == b.params.keys() and all(torch.equal(a.params[k], b.params[k]) for k in a.params)
    for u, v in zip([a.x] + a.V + a.U + list(a.Hsrc.values()), [b.x] + b.V + b.U + list(b.Hsrc.values())):
        assert torch.equal(u, v)
    steps, taps, pairs = a
    assert steps is a.steps and taps == a.taps and pairs == a.pairs


def test_census():
    """every listed feature at least once in the exact corpus, every motif at least twice and every way of composing them in the real corpus"""
    exact = [R.census(R.tape("exact", s)) for s in R.EXACT_SEEDS]
    real = [R.census(R.tape("real", s)) for s in R.REAL_SEEDS]
    for f in R.EXACT_FEATURES:
        assert sum(f in c for c in exact) >= 1, f"no exact tape reaches {f}"
    for m in R.REAL_MOTIFS:
        assert sum(m in c for c in real) >= 2, f"motif {m} occurs in fewer than two real tapes"
    for m in R.REAL_COMPOSITIONS + ("tap_mid", "fan2", "fan3", "res_first", "res_second", "concat_inactive", "hw60", "cin4"):
        assert sum(m in c for c in real) >= 1, f"no real tape reaches {m}"
    assert {(g.B, g.kps) for g in map(lambda s: R.tape("exact", s), R.EXACT_SEEDS)} == {(2, 2), (1, 3)}
    assert {(R.tape("real", s).B, R.tape("real", s).kps) for s in R.REAL_SEEDS} == {(2, 2), (1, 3)}
    assert {R.tape("exact", s).hw for s in R.EXACT_SEEDS} == set(R.EXACT_SHAPES)
    assert all(len(R.tape("exact", s).steps) <= 9 for s in R.EXACT_SEEDS)
    for s in R.REAL_SEEDS:                              # the transformer block at C = 320 on 60 rows: M = 240 with four tangents
        g = R.tape("real", s)
        if "tf" in g.motifs:
            assert g.hw == (6, 10) and any(R.kind(st) == "ln" and g.meta[st["src"]][0] == 320 for st in g.steps) and 60 * g.nt >= 180


@pytest.mark.parametrize("seed", R.EXACT_SEEDS)
def test_exact_precondition_and_identity(seed):
    g = R.tape("exact", seed)
    assert R.check_exact_precondition(g) < 2.0 ** 8
    ref = R.reference(g, F32)
    for dtype in (BF, F16):                             # rounding a stored buffer changes nothing: one corpus serves the three dtypes
        st = R.flat_results(R.reference(g, dtype, store=dtype))
        for k, v in R.flat_results(ref).items():
            assert torch.equal(st[k], v), (seed, dtype, k)
    q = 4.0 ** R.pools(g)
    for p in range(len(g.passes)):                      # <U, J V> = <J^T U, V> as integers (times 4^-P)
        a, b = (g.U[p].double() * ref["jvp"][p]).sum() * q, (ref["vjp"][p] * g.V[p].double()).sum() * q
        assert a == b and a == a.round(), (seed, g.passes[p], float(a), float(b))


@pytest.mark.parametrize("seed", R.REAL_SEEDS)
def test_real_reference_against_finite_differences(seed):
    """central differences (fp64, h = 1e-6: truncation ~1e-12, rounding ~1e-10 of the values) for every pass, and the adjoint identity"""
    g = R.tape("real", seed)
    ref = R.reference(g, F32)
    x, ctx = R._rx(g, F32)
    idx = torch.arange(g.nt) // g.kps
    xs, cs = x[idx], (ctx[idx] if ctx is not None else None)
    with torch.no_grad():
        full = R.evaluate(g, F32, x, ctx)
        h = 1e-6
        for p, (src, dst) in enumerate(g.passes):
            V, U = g.V[p].double(), g.U[p].double()
            f = lambda t: R.evaluate(g, F32, xs, cs, override={src: t})[dst]
            fd = (f(full[src][idx] + h * V) - f(full[src][idx] - h * V)) / (2 * h)
            assert float((fd - ref["jvp"][p]).norm() / ref["jvp"][p].norm()) < 1e-6, (seed, src, dst)
            a, b = float((U * ref["jvp"][p]).sum()), float((ref["vjp"][p] * V).sum())
            assert abs(a - b) <= 1e-9 * max(abs(a), abs(b)), (seed, src, dst, a, b)


def test_drop_instances_cover_every_kind():
    exact = [f[0] for s in R.EXACT_SEEDS for f in R.feature_instances(R.tape("exact", s))]
    real = [f[0] for s in R.REAL_SEEDS for f in R.feature_instances(R.tape("real", s))]
    assert all(exact.count(k) >= 5 for k in ("consumer", "residual", "window")), {k: exact.count(k) for k in set(exact)}
    assert all(real.count(k) >= 5 for k in ("consumer", "residual", "window", "sample")), {k: real.count(k) for k in set(real)}


def _moved(ref, bad, feature, exact):
    """largest change over the results the feature can touch: elements that differ (exact tier) or the row error (real tier)"""
    r, b = R.flat_results(ref), R.flat_results(bad)
    worst = {}
    for name in r:
        if name.split(":")[0] in R.affected(feature):
            w = float((r[name] != b[name]).sum()) if exact else R.errors(b[name], r[name])[0]
            worst[R.pass_of(name)] = max(worst.get(R.pass_of(name), 0.0), w)
    return worst


@pytest.mark.parametrize("seed", R.EXACT_SEEDS)
def test_exact_drop_is_visible(seed):
    g = R.tape("exact", seed)
    ref = R.reference(g, F32)
    for f in R.feature_instances(g):                    # (a plain chain has none)
        assert max(_moved(ref, R.drop(g, F32, f), f, True).values()) >= 1, f"seed {seed}: dropping {f} changes no output element"


@pytest.mark.parametrize("seed", R.REAL_SEEDS)
def test_real_drop_is_visible(seed):
    """every dropped contribution moves the row error of a pass above that pass's bound, in every dtype's scale (the loosest is bf16's)"""
    g = R.tape("real", seed)
    ref = R.reference(g, F32)
    inst = R.feature_instances(g)
    assert any(f[0] == "consumer" for f in inst) and any(f[0] == "residual" for f in inst)
    for f in inst:
        moved = _moved(ref, R.drop(g, F32, f), f, False)
        for dtype in (F32, F16, BF):
            assert any(w > R.BOUNDS[(dtype, which)] for which, w in moved.items()), f"seed {seed}: dropping {f} moves the row errors by {moved} only"
