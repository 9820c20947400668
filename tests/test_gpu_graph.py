"""The engine's graph bookkeeping on random small tapes (tests/_graph_ref.py) against an fp64 restatement, on the device.

1. Exact tier: 40 tapes x {fp32, bf16, fp16}; primal at every tap, jvp / vjp from x, jvp_between / vjp_between, forward and forward_from are bit
   for bit ref64.float().to(dtype), under the split-K heuristic and under a forced split of 3.  No tolerance.
2. Real tier: 12 tapes x 3 dtypes, the same passes, by row against fp64 (the row error of _norm_ref).  Three arms per tape: the defaults; "off"
   (lazy_reduce = 0, ln_fuse = 0, geglu_fwd = 0, cross_fold = 0); "on" (ln_fuse = 1, cross_fold = 2, gemm_tile = 515: ln_fuse is off by default,
   the default cross_fold rule folds no layer below C = 640, and the heuristic gives the GEGLU epilogues' ring tile to products of some 400
   tiles only, so at 60 rows the three routes are reached only when forced).  `test_real_toggles_reached` asserts that each of the four
   switches, flipped alone (geglu_fwd: on the forced ring tile), changes the launch count of at least one tape.  BOUNDS are twice the largest row error measured
   over the corpus and the arms; G guards against having measured a wrong engine: the engine's global error is at most G x the global error of
   the restatement that rounds every stored buffer to the dtype (the error of an ideal engine), G twice the largest measured ratio.  fp32: the
   adjoint identity <U, J V> = <J^T U, V> to 1e-4 relative.
3. State independence, no reference: a seeded sequence of about 20 calls on ONE engine per tape, primal and forward calls on two inputs; every result equals, bit for bit, the same
   call issued right after its primal on a fresh engine, and iterate equals orth(vjp(jvp(V))) under iter_alias 1 and 0 (three iterations: all
   but the last lend T(tap) to G(tap), the second on top of what the first left behind).

Measured on an MI355X: the largest row error over the 12 tapes, their passes and the 3 arms (BOUNDS is twice that), the ideal-engine emulation's
largest global error, and the largest ratio of the engine's global error to the emulation's on the same result (G is twice that):
    dtype  pass      row error   emulation (global)   ratio
    fp32   primal    6.7e-07     6.4e-08              8.9
    fp32   tangent   1.1e-06     8.8e-08              8.5
    fp32   adjoint   4.0e-06     8.5e-08              9.6      G = 19.1
    bf16   primal    9.7e-03     4.3e-03              1.2
    bf16   tangent   1.8e-02     5.9e-03              1.2
    bf16   adjoint   4.5e-02     6.0e-03              1.7      G = 3.3
    fp16   primal    1.2e-03     5.3e-04              1.3
    fp16   tangent   1.7e-03     7.0e-04              1.2
    fp16   adjoint   4.6e-03     6.6e-04              1.7      G = 3.5
(fp32: the emulation rounds stored buffers only, the engine also accumulates its products in fp32 -- hence the larger ratio.  The arms differ by
less than 1 % in their maxima.  The largest row errors are the adjoint's at x: rows of the 4-channel input whose cotangent nearly cancels; the
emulation shows the same rows, 4.4e-02 in bf16.)
The file takes 12 s on an MI355X (224 tests); the longest test is the first one, 2.0 s with the start of the runtime, every other below 0.4 s.
Checked against eleven planted bookkeeping mistakes in a scratch build of engine.cpp (an un-zeroed concat window, a residual or a second consumer
that overwrites, skip / ginit not reset, the inactive-input product run anyway, the parked product not flushed or not stored, ...): nine fail
this file at its first affected tape; the two that pass change no result the API can reach (g_off left swapped between same-sized buffers;
fold_live left on, whose operands the next covering primal rebuilds).
"""
import contextlib
import random

import pytest
import torch

import _graph_ref as R
from _graph_ref import BF, F16, F32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = [pytest.param(F32, id="fp32"), pytest.param(BF, id="bf16"), pytest.param(F16, id="fp16")]
DEFAULTS = dict(gemm_tile=0, gemm_splitk=0, lazy_reduce=1, ln_fuse=0, geglu_fwd=1, cross_fold=1, iter_alias=1)     # dpb_debug_set has no getter: engine.cpp's initial values
RING = dict(gemm_tile=515)                            # the BK = 64 ring forced: the GEGLU epilogues fuse on it at any M (the heuristic wants some 400 tiles of 128 x 128)
ARMS = {"default": {}, "off": dict(lazy_reduce=0, ln_fuse=0, geglu_fwd=0, cross_fold=0), "on": dict(ln_fuse=1, cross_fold=2, **RING)}
TOGGLES = {"lazy_reduce": ({}, dict(lazy_reduce=0)), "ln_fuse": (dict(ln_fuse=1), dict(ln_fuse=0)),      # (route reached, route off)
           "geglu_fwd": (RING, dict(geglu_fwd=0, **RING)), "cross_fold": (dict(cross_fold=2), dict(cross_fold=0))}

BOUNDS, G = R.BOUNDS, R.G                            # twice the measured maxima (module docstring); the host tests use them as the scale of a visible error


@contextlib.contextmanager
def debug(**kw):
    from diffusion_pullback_amd import lib as L
    lib = L.load()
    try:
        for k, v in kw.items():
            L.check(lib.dpb_debug_set(k.encode(), int(v)))
        yield
    finally:
        for k in kw:
            L.check(lib.dpb_debug_set(k.encode(), DEFAULTS[k]))


_REF = {}


def ref_of(tier, seed, dtype, store=None):
    """computed once, shared, left unchanged (the exact tier's reference does not depend on the dtype: every value is exact in all three)"""
    key = (tier, seed, None if tier == "exact" else dtype, store)
    if key not in _REF:
        _REF[key] = R.flat_results(R.reference(R.tape(tier, seed), F32 if tier == "exact" else dtype, store=store))
    return _REF[key]


def run(g, dtype, **settings):
    """a fresh engine, every call of _graph_ref.run_engine -> ({name: fp32 cpu tensor}, {call: launches})"""
    with debug(**settings):
        e = R.engine(g, dtype, DEV)
        out, n = R.run_engine(e, g, R.device_inputs(g, dtype, DEV))
        out = {k: v.cpu() for k, v in R.flat_results(out).items()}
        del e
    return out, n


# =============================================================================================== 1. exact tier
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("seed", R.EXACT_SEEDS)
def test_exact(seed, dtype):
    g = R.tape("exact", seed)
    ref = ref_of("exact", seed, dtype)
    for arm, settings in (("heuristic", {}), ("splitk3", dict(gemm_splitk=3))):
        out, _ = run(g, dtype, **settings)
        for name, want in ref.items():
            R.compare_exact(out[name], R.rnd(want, dtype), f"exact seed {seed} {str(dtype)[6:]} {arm} {name}")


# =============================================================================================== 2. real tier
def measure_real(seed, dtype, arms=ARMS):
    """-> {arm: {name: (row error, global error, emulation's global error)}}, {arm: launches}, {arm: results}"""
    g = R.tape("real", seed)
    ref, emu = ref_of("real", seed, dtype), ref_of("real", seed, dtype, store=dtype)
    fig, launches, results = {}, {}, {}
    for arm, settings in arms.items():
        out, launches[arm] = run(g, dtype, **settings)
        results[arm] = out
        fig[arm] = {name: R.errors(out[name], ref[name]) + (R.errors(emu[name], ref[name])[1],) for name in ref}
    return fig, launches, results


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("seed", R.REAL_SEEDS)
def test_real(seed, dtype):
    g = R.tape("real", seed)
    fig, _, results = measure_real(seed, dtype)
    bad = []
    for arm, f in fig.items():
        for name, (row, glob, emu) in f.items():
            print(f"real seed {seed} {str(dtype)[6:]} {arm} {name}: row {row:.3e} global {glob:.3e} emulation {emu:.3e} ratio {glob / emu:.2f}")
            if row > BOUNDS[(dtype, R.pass_of(name))]:
                bad.append(f"{arm} {name}: row error {row:.3e} > {BOUNDS[(dtype, R.pass_of(name))]:.1e}")
            if glob > G[dtype] * emu:
                bad.append(f"{arm} {name}: global error {glob:.3e} > G = {G[dtype]} x the ideal engine's {emu:.3e}")
    assert not bad, f"real seed {seed} {str(dtype)[6:]}: " + "; ".join(bad)
    if dtype == F32:
        for arm, out in results.items():
            for p in range(len(g.passes)):
                a = float((out[f"jvp:{p}"].double() * R.rnd(g.U[p], dtype).double()).sum())
                b = float((out[f"vjp:{p}"].double() * R.rnd(g.V[p], dtype).double()).sum())
                assert abs(a - b) <= 1e-4 * max(abs(a), abs(b)), f"real seed {seed} {arm} pass {g.passes[p]}: <U, J V> = {a!r}, <J^T U, V> = {b!r}"


@pytest.mark.parametrize("toggle", list(TOGGLES))
def test_real_toggles_reached(toggle):
    """the switch, flipped alone, changes the launch count of at least one bf16 tape: the corpus reaches the route it controls"""
    on, off = TOGGLES[toggle]
    for seed in R.REAL_SEEDS:
        g = R.tape("real", seed)
        if not ({"tf", "cross"} & set(g.motifs)):
            continue
        _, a = run(g, BF, **on)
        _, b = run(g, BF, **off)
        if a != b:
            print(f"{toggle}: seed {seed} differs in", {k: (a[k], b[k]) for k in a if a[k] != b[k]})
            return
    raise AssertionError(f"no tape's launch count depends on {toggle}: the corpus never reaches that route")


# =============================================================================================== 3. state independence
def _same(a, b) -> bool:
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))      # (bit for bit: a NaN equals itself)


class _Driver:
    """issues a call on an engine; the same code serves the long-lived engine and the fresh ones"""

    def __init__(self, g, dtype, seed):
        self.g, self.dtype = g, dtype
        self.tp = R.build_tape(g, dtype, DEV)
        self.io = R.device_inputs(g, dtype, DEV)
        gen = torch.Generator().manual_seed(seed)
        mk = lambda shape: R.rnd(torch.randn(*shape, generator=gen), dtype).to(DEV)
        self.Ux = {t: mk(g.shape(t, g.nt)) for t in g.taps}                       # cotangents of the x-seeded pass to every tap
        v0 = torch.randn(g.nt, g.cin * g.hw[0] * g.hw[1], generator=gen)
        self.V0 = (v0 / v0.norm(dim=1, keepdim=True)).to(DEV)
        # a second input: state derived from the primal (statistics, affine tables, folded operands) must follow the input of the primal in force
        x2 = -self.io["x"] if g.tier == "exact" else mk(g.shape("x", g.B))
        self.xs = [(self.io["x"], self.io["ctx"]), (x2, self.io["ctx"].flip(1).contiguous() if g.ctx else None)]

    def engine(self):
        from diffusion_pullback_amd.engine import Engine
        rb = any(R.kind(s) == "conv" and s["rowbias"] for s in self.g.steps)
        return Engine(self.tp, R.TEMB if rb else 8, False, True, self.g.cin, max_batch=self.g.B, max_tangents=self.g.nt)

    def covered(self, upto):
        return [t for t in self.g.taps if self.g.producer(t) <= self.g.producer(upto)]

    def call(self, e, c):
        g, io = self.g, self.io
        k = c[0]
        if k == "primal":
            x, ctx = self.xs[c[2]]
            e.primal(x, g.t, ctx, c[1])
            return [e.read(t).clone() for t in self.covered(c[1])]
        if k == "jvp":
            return [e.jvp(c[1], io["V"][0].reshape(g.nt, -1)).clone()]
        if k == "vjp":
            return [e.vjp(c[1], self.Ux[c[1]].reshape(g.nt, -1)).clone()]
        if k == "jvp_between":
            p = c[1]
            return [e.jvp_between(*g.passes[p], io["V"][p].reshape(g.nt, -1)).clone()]
        if k == "vjp_between":
            p = c[1]
            return [e.vjp_between(*g.passes[p], io["U"][p].reshape(g.nt, -1)).clone()]
        if k == "forward":
            x, ctx = self.xs[c[2]]
            return [e.forward(x, g.t, ctx, c[1]).clone()]
        if k == "from":
            src, dst = g.pairs[c[1]]
            x, ctx = self.xs[c[2]]
            return [e.forward_from(x, g.t, ctx, src, io["H"][src], dst).clone()]
        if k == "iterate":
            with debug(iter_alias=c[1]):
                return [t.clone() for t in e.iterate(g.last, self.V0.clone(), 3)]
        raise ValueError(c)

    def composed_iterate(self, e):
        """three power iterations from the public pieces: orth(vjp(jvp(V))) per sample"""
        g = self.g
        V = self.V0.clone()
        for _ in range(3):
            U = e.jvp(g.last, V)
            W = e.vjp(g.last, U)
            parts = [e.orth(W[b * g.kps:(b + 1) * g.kps].contiguous(), V[b * g.kps:(b + 1) * g.kps].contiguous()) for b in range(g.B)]
            V = torch.cat([p[0] for p in parts])
        return [V, U, torch.cat([p[1] for p in parts]), torch.stack([p[2] for p in parts])]


def _sequence(g, rng):
    """about 20 calls in mixed order; a derivative call only to a tap the primal in force covers (the engine keeps activations up to there)"""
    seq, upto = [("primal", g.last, 0)], g.last
    kinds = ["jvp", "vjp", "jvp_between", "vjp_between", "primal", "forward", "from", "iterate"]
    iters = [1, 0]
    while len(seq) < 20:
        k = rng.choice(kinds)
        cov = [t for t in g.taps if g.producer(t) <= g.producer(upto)]
        if k == "primal":
            upto = rng.choice(g.taps)
            seq.append(("primal", upto, rng.randrange(2)))
        elif k in ("jvp", "vjp"):
            seq.append((k, rng.choice(cov)))
        elif k in ("jvp_between", "vjp_between"):
            p = rng.randrange(1, len(g.passes))
            if g.passes[p][1] in cov:
                seq.append((k, p))
        elif k == "iterate":
            if upto == g.last and iters:
                seq.append(("iterate", iters.pop()))
        else:
            seq.append(("forward", rng.choice(g.taps), rng.randrange(2)) if k == "forward" else ("from", rng.randrange(len(g.pairs)), rng.randrange(2)))
            seq.append(("refused",))
            upto = rng.choice(g.taps)
            seq.append(("primal", upto, rng.randrange(2)))
    return seq


STATE_CASES = [("exact", s, "default") for s in R.EXACT_SEEDS] + [("real", s, arm) for s in R.REAL_SEEDS for arm in ("default", "on")]


@pytest.mark.parametrize("tier,seed,arm", STATE_CASES, ids=[f"{t}{s}-{a}" for t, s, a in STATE_CASES])
def test_state_independence(tier, seed, arm):
    """real tier: under the defaults and with the fused epilogues and the folded attention forced (the ops they swallow are skipped per pass)"""
    with debug(**ARMS[arm]):
        _state_independence(tier, seed)


def _state_independence(tier, seed):
    from diffusion_pullback_amd import lib as L
    g = R.tape(tier, seed)
    dtype = (F32, BF, F16)[seed % 3] if tier == "exact" else BF
    d = _Driver(g, dtype, 977 * seed + 5)
    seq = _sequence(g, random.Random(31 * seed + (7 if tier == "real" else 0)))
    e = d.engine()
    fresh = {}
    upto = None                                         # the primal in force: (tap, input)
    for i, c in enumerate(seq):
        what = f"{tier} seed {seed} call {i} {c} after primal (tap, input) {upto}"
        if c[0] == "refused":                           # forward / forward_from keep no stash: a derivative pass has nothing to linearise at
            with pytest.raises(L.DpbError):
                e.jvp(g.last, d.io["V"][0].reshape(g.nt, -1))
            continue
        got = d.call(e, c)
        if c[0] == "primal":
            upto = c[1:]
        key = (c, upto if c[0] not in ("primal", "forward", "from") else None)
        if key not in fresh:
            f = d.engine()
            if key[1] is not None:
                d.call(f, ("primal",) + key[1])
            fresh[key] = d.call(f, c)
            if c[0] == "iterate":
                f2 = d.engine()
                d.call(f2, ("primal",) + upto)
                for j, (a, b) in enumerate(zip(fresh[key], d.composed_iterate(f2))):
                    assert _same(a, b), f"{what}: iterate output {j} (V, U, s, conv) differs from orth(vjp(jvp(V)))"
        assert len(got) == len(fresh[key])
        for j, (a, b) in enumerate(zip(got, fresh[key])):
            assert _same(a, b), f"{what}: result {j} differs from the same call on a fresh engine ({int((a.cpu() != b.cpu()).sum())} of {a.numel()} elements)"
