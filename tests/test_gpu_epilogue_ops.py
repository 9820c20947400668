"""The fused product epilogues of csrc/epilogue.h (and their twins in gemm_p8.hip) -- EPI_GEGLU_TAN, EPI_GEGLU_ADJ, EPI_GEGLU_FWD, EPI_LN_TAN, EPI_LN_ADJ --
at op level against the fp64 reference of tests/_norm_ref.py: tiny tapes (tests/_epilogue_ref.py) whose FF-in product asks for the 64-interleaved
weight layout, so that `geglu_next` / `geglu_prev` are set, and 320-wide products around a LayerNorm under dpb_debug_set("ln_fuse", 1 | 3); primal,
tangent, adjoint and dpb_forward, under every forced tile code whose kernel is built with the epilogues, the heuristic, and the codes that must not
fuse.  Every row of every output is compared.

Nets.  G3: h = linear(x, 2F, interleave = 64), y = geglu(h, il = 64), o = linear(y, C); G2: the first two steps, tap on y.  x is scaled by 3 (the
gate covers both GELU tails).  L1: h = linear(x[K], 320), z = ln(h), o = linear(z, Cout); L2: h = linear(x, 320) + linear(x, 320) (the tangent epilogue
adds R before it rounds); L3: o = concat(linear(z, Cout), h) (h has a later reader: the adjoint epilogue accumulates onto the concat's cotangent and
the tangent's C store is read back).  Shapes: rows = 77 with (B, kps) = (2, 2): M = 308 -- sample boundaries inside 32-row slabs, two full and one
ragged 128-row tile, one full and one ragged 256-row tile, ragged against the 64-row steps of the row-complete tile; rows = 7: M = 28, less than one
slab; (1, 1) and (1, 3): a wrong j / kps mapping reads another sample's stash; C = 72: K is no multiple of either ring's BK, C = 64: exactly one K
tile; F = 64, 128, 192, 256: tangent N = 128 .. 512, adjoint N = 64 .. 256.

Reference.  The interleave only permutes the rows of the FF-in weight and GEGLU undoes it, so the reference of an interleaved net is
_norm_ref.reference of the same net with il = 0 (tests/test_epilogue_ops_host.py asserts the identity in fp64).  That net on the engine is the
"base arm": it can never fuse, and its kernels are pinned by test_gpu_product_ops.py and test_gpu_norm_ops.py.  For the LayerNorm nets the base arm
is the same engine under ln_fuse = 0.

Route proof.  _epilogue_ref restates the rule of gemm_epi_supported / pick_async_tile (checked against dpb_debug_gemm_plan by the host file): the
tangent fuses iff the engine is 16-bit, 2F % 128 == 0, the tile that runs the product is built with the epilogues (TILE_GEGLU) and made of whole
128-column blocks, and 2F % 256 == 0 on the 256-column tiles (518, 530); the adjoint the same with F; dpb_forward the same as the tangent when the
plain product would run unsplit.  A fusing pass must launch exactly one kernel fewer than the base arm, a pass the rule marks unfused exactly as
many (code 65; F = 64 or 192 in the adjoint; F = 192 on 518 / 530; the heuristic at K = 72; any fp32 engine), and with profiling on every product's
bracket has the kind include/dpb.h documents for the forced code.  A forced gemm_splitk = 3 adds one launch per unfused product and none for a fused
one.  LayerNorm: one launch fewer per fused LayerNorm and pass than under ln_fuse = 0 (tangent: M >= 128 and K % 64 == 0; adjoint: M >= 128, Cout % 64
== 0 and Cout <= 1024 unless ln_fuse & 2).
Code 521 (the 64 x 128 half tile) is not built with the epilogues; the dispatch does not leave its FF-in product unfused but hands it to the row's
documented substitute, 515, where it fuses (include/dpb.h: "the substitute row that runs a product the forced tile does not take";
tests/golden/gemm_plans.npz pins exactly that plan).  So under 521 the rule -- and this file -- expect the fused launch count, on tile 515.

dpb_forward: bitwise primal() + read, bitwise the geglu_fwd = 0 arm, one launch fewer than that arm where the rule says fused (engine.cpp and
epilogue.h promise both equalities; no tolerance).

Not reachable at op level, hence not tested: accumulate = 1 in EPI_GEGLU_ADJ (the engine refuses a GEGLU input with a second consumer) and
alpha != 1 there (no tape op scales a product), and a residual in EPI_GEGLU_TAN (an FF-in product with a residual never gets geglu_next).

Bounds (_norm_ref.BOUNDS, families epi_geglu, epi_geglu_fwd, epi_ln): twice the largest error measured on an MI355X over all the cases of a family
(fused and unfused routes alike); row error as in test_gpu_norm_ops.py.  Guard against having measured a wrong kernel: the fused routes round once
less than the unfused ones, so the largest error of the fused launches must be at most 1.25 x the largest error of the base arm on the same cases:
asserted per test on the global error, and over the whole family on row and global error by the last test of the file (a row maximum is the extreme
of a few hundred rows of ONE case: within the test of F = 64, bf16, the fused tangent's 7.3e-03 stands against 5.7e-03, over the family against
6.8e-03, while the global error of a fused GEGLU pass is at most 0.94 x the base arm's in every one of the 518 cases).  Measured maxima, row / global,
primal | tangent | adjoint (forward: one column); "all": every case of the family, fused or not -- half the bound; "fused": the passes the rule
marks fused; "base": the base arm on those same cases.  The LayerNorm epilogues round h / the cotangent to 16 bit exactly where the separate
kernels store them, so their arms agree to the digits shown; the launch count tells them apart.
    fp32 epi_geglu     all   4.2e-07 / 3.0e-07 | 4.9e-07 / 3.1e-07 | 4.8e-07 / 3.6e-07
    bf16 epi_geglu     all   6.2e-03 / 3.5e-03 | 7.3e-03 / 3.6e-03 | 6.6e-03 / 3.6e-03
    bf16 epi_geglu     fused        --         | 7.3e-03 / 3.3e-03 | 5.1e-03 / 3.2e-03
    bf16 epi_geglu     base         --         | 6.8e-03 / 3.7e-03 | 5.7e-03 / 3.6e-03
    fp16 epi_geglu     all   6.9e-04 / 4.4e-04 | 8.6e-04 / 4.5e-04 | 8.2e-04 / 4.5e-04
    fp16 epi_geglu     fused        --         | 6.8e-04 / 4.2e-04 | 6.5e-04 / 4.0e-04
    fp16 epi_geglu     base         --         | 8.6e-04 / 4.6e-04 | 8.2e-04 / 4.6e-04
    fp32 epi_geglu_fwd all   4.2e-07 / 3.0e-07
    bf16 epi_geglu_fwd all   6.2e-03 / 3.5e-03
    bf16 epi_geglu_fwd fused 6.2e-03 / 3.5e-03
    bf16 epi_geglu_fwd base  6.2e-03 / 3.5e-03
    fp16 epi_geglu_fwd all   6.9e-04 / 4.4e-04
    fp16 epi_geglu_fwd fused 6.9e-04 / 4.4e-04
    fp16 epi_geglu_fwd base  6.9e-04 / 4.4e-04
    fp32 epi_ln        all   5.0e-07 / 3.5e-07 | 5.7e-07 / 3.9e-07 | 4.6e-07 / 3.6e-07
    bf16 epi_ln        all   4.0e-03 / 3.0e-03 | 4.5e-03 / 3.2e-03 | 4.2e-03 / 3.1e-03
    bf16 epi_ln        fused        --         | 4.5e-03 / 3.2e-03 | 4.2e-03 / 3.1e-03
    bf16 epi_ln        base         --         | 4.5e-03 / 3.2e-03 | 4.2e-03 / 3.1e-03
    fp16 epi_ln        all   5.0e-04 / 3.7e-04 | 5.8e-04 / 4.1e-04 | 5.4e-04 / 4.0e-04
    fp16 epi_ln        fused        --         | 5.8e-04 / 4.1e-04 | 5.1e-04 / 4.0e-04
    fp16 epi_ln        base         --         | 5.8e-04 / 4.1e-04 | 5.1e-04 / 4.0e-04
The file: 27 tests in about 7 s on an MI355X, the longest 3.2 s (the first, which loads the library), every other 0.1 s or less.  No kernel bug was
found.
"""
import csv
import time
import zlib

import pytest
import torch

import _epilogue_ref as E
import _norm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F16, F32 = R.BF, R.F16, R.F32
D16 = [pytest.param(BF, id="bf16"), pytest.param(F16, id="fp16")]
NAME = {F32: "fp32", BF: "bf16", F16: "fp16"}
PASSES = E.PASSES
_PREP = {}                                              # inputs and fp64 references per (net, shape, dtype): computed once for all codes and tests


def _set(key: str, value: int):
    from diffusion_pullback_amd import lib as L
    L.check(L.load().dpb_debug_set(key.encode(), value))


def _prepared(tag, ref_steps, make_params, cin, cout, rows, B, kps, dtype, scale):
    key = (tag, cin, cout, rows, B, kps, dtype)
    if key not in _PREP:
        g = torch.Generator().manual_seed(zlib.crc32(repr((tag, cin, rows, B, kps)).encode()))
        params = make_params(g)
        nt = B * kps
        x = R.plain_input(g, (B, rows, cin), dtype, scale).to(DEV)
        V = R.plain_input(g, (nt, rows, cin), dtype).to(DEV)
        U = R.plain_input(g, (nt, rows, cout), dtype).to(DEV)
        _PREP[key] = (params, x, V, U, R.reference(ref_steps, params, x, dtype, V, U, kps))
    return _PREP[key]


def _check(acc, out, ref, family, dtype, p, arm, label, bounded=True):
    """one output against the fp64 reference: prints the EPI-ERR line, collects the maxima per (family, pass, arm), asserts the family's bound"""
    e = R.row_errors(out.to(ref.device), ref)
    row = float(e.max())
    glob = float((out.to(ref.device).double() - ref).norm() / ref.norm().clamp_min(1e-300))
    print(f"EPI-ERR {family} {NAME[dtype]} {p} {arm} {label} row={row:.3e} glob={glob:.3e}")
    m = acc.setdefault((family, p, arm), [0.0, 0.0])
    m[0] = max(m[0], row); m[1] = max(m[1], glob)
    if bounded:
        rb, gb = R.bound(family, dtype, "primal" if p == "forward" else p)
        if not (row <= rb and glob <= gb):
            R.compare(out, ref, 0, rb, gb, f"{p} {family} {NAME[dtype]} {arm} {label}")
            raise AssertionError(f"{p} {family} {NAME[dtype]} {arm} {label}: non-finite error figures {row} / {glob}")


_ACC, _DONE = {}, {}                                    # the maxima of the whole session per (family, dtype, pass, arm); the tests that fed them
TESTS_PER_DTYPE = {"geglu": 9, "ln": 3}                 # the 16-bit tests of a group: the family-wide guard waits for all of them


def _guard(acc, dtype, group, name):
    """The fused launches round once less than the base arm.  Per test: their largest GLOBAL error (a mean over every element: a stable figure) may
    not exceed 1.25 x the base arm's on the same cases.  The maxima go into the session's table for the family-wide guard on the row maxima too."""
    for (family, p, arm), m in acc.items():
        s = _ACC.setdefault((family, dtype, p, arm), [0.0, 0.0])
        s[0] = max(s[0], m[0]); s[1] = max(s[1], m[1])
        if arm == "fused":
            u = acc[(family, p, "base+")][1]
            assert m[1] <= 1.25 * u, f"{family} {NAME[dtype]} {p}: fused global maximum {m[1]:.3e} > 1.25 x the base arm's {u:.3e} on the same cases"
    _DONE.setdefault((group, dtype), set()).add(name)


def _kinds(e, path, run):
    """runs `run` with profiling on -> its result and the (kind, N) of every product bracket"""
    e.profile(True)
    try:
        out = run()
        e.profile_dump(str(path))
    finally:
        e.profile(False)
    with open(path) as fh:
        return out, [(int(r["big"]), int(r["N"])) for r in csv.DictReader(fh)]


def _forward(e, x):
    O, _, _, n = R.run_engine(e, x, None, None, forward_only=True)
    return O, n["primal"]


# =============================================================================================== GEGLU
def _geglu_case(acc, kind, dtype, F, C, rows, B, kps, codes, tmp_path):
    """G3 / G2 with il = 64 (and the il = 0 base arm) under each code: errors, launch counts, bracket kinds, forced split, dpb_forward"""
    nt = B * kps
    params, x, V, U, ref = _prepared(kind + f"F{F}", E.geglu_net(kind, F, C, 0), lambda g: E.geglu_params(g, F, C), C, C if kind == "G3" else F,
                                      rows, B, kps, dtype, 3.0)
    e64 = R.engine(R.build_tape(E.geglu_net(kind, F, C, 64), params, dtype, DEV, rows, C), B, nt)
    e0 = R.engine(R.build_tape(E.geglu_net(kind, F, C, 0), params, dtype, DEV, rows, C), B, nt)
    products = 2 if kind == "G3" else 1                              # per pass
    try:
        for code in codes:
            exp = E.geglu_expected(kind, dtype, code, F, C, rows, B, kps)
            label = f"{kind} F={F} C={C} rows={rows} B={B} kps={kps} code={code}"
            # the base arm's plain product may split K by itself (the heuristic at K = 2048): its reduce launch goes with the GEGLU launch
            red = {p: int(bool(exp[p]) and E.plain_split(dtype, code, nt * rows, N, C) > 1) for p, N in (("primal", 0), ("tangent", 2 * F), ("adjoint", F))}
            _set("gemm_tile", code); _set("gemm_splitk", 0)
            (O, dO, gX, n), kinds = _kinds(e64, tmp_path / "p.csv", lambda: R.run_engine(e64, x, V, U))
            O0, dO0, gX0, n0 = R.run_engine(e0, x, V, U)
            # ---- route: launch counts against the base arm, bracket kinds
            for p in PASSES:
                assert n0[p] - n[p] == exp[p] + red[p], (f"{label} {NAME[dtype]} {p}: {n[p]} launches, the il = 0 arm {n0[p]}; the rule expects "
                                                         f"{exp[p] + red[p]} fewer (a silent route change)")
            assert len(kinds) == 3 * products, (label, kinds)
            if kind == "G3":
                assert [k[1] for k in kinds] == [2 * F, C, 2 * F, C, F, C], (label, kinds)
            if dtype == F32:
                assert all(k[0] in (0, 1) for k in kinds), (label, kinds)
            elif code:
                assert all(k[0] == E.TILES[code][3] for k in kinds), f"{label}: brackets {kinds}, expected kind {E.TILES[code][3]} throughout"
            else:
                fused = [kinds[products]] * exp["tangent"] + [kinds[2 * products]] * exp["adjoint"]
                assert all(k[0] == 4 for k in fused), f"{label}: the fused products' brackets {fused}, expected the BK = 64 ring (kind 4)"
            # ---- errors of both arms
            for p, out, base, r in zip(PASSES, (O, dO, gX), (O0, dO0, gX0), ref):
                _check(acc, out, r, "epi_geglu", dtype, p, "fused" if exp[p] else "unfused", label)
                _check(acc, base, r, "epi_geglu", dtype, p, "base+" if exp[p] else "base-", label, bounded=False)
            # ---- a forced split leaves the fused product whole: one more launch per unfused product only
            _set("gemm_splitk", 3)
            O3, dO3, gX3, n3 = R.run_engine(e64, x, V, U)
            _set("gemm_splitk", 0)
            for p, out, r in zip(PASSES, (O3, dO3, gX3), ref):
                assert (not code and C >= 256) or n3[p] - n[p] == products - exp[p], (f"{label} {NAME[dtype]} {p}: {n3[p]} launches at gemm_splitk 3, {n[p]} unsplit; expected "
                                                           f"{products - exp[p]} more ({exp[p]} fused product(s) stay whole)")
                _check(acc, out, r, "epi_geglu", dtype, p, "fused" if exp[p] else "unfused", label + " splitk=3")
            # ---- dpb_forward: bitwise primal + read, bitwise the geglu_fwd = 0 arm, one launch fewer where fused
            Of, nf = _forward(e64, x)
            _set("geglu_fwd", 0)
            Og, ng = _forward(e64, x)
            _set("geglu_fwd", 1)
            assert torch.equal(Of, O), f"{label} {NAME[dtype]}: forward() differs from primal() + read in {(Of != O).sum().item()} elements"
            assert torch.equal(Of, Og), f"{label} {NAME[dtype]}: forward() differs from its geglu_fwd = 0 arm in {(Of != Og).sum().item()} elements"
            assert ng - nf == exp["forward"], f"{label} {NAME[dtype]}: forward {nf} launches, geglu_fwd = 0 {ng}; the rule expects {exp['forward']} fewer"
            _check(acc, Of, ref[0], "epi_geglu_fwd", dtype, "forward", "fused" if exp["forward"] else "unfused", label)
            _check(acc, O0, ref[0], "epi_geglu_fwd", dtype, "forward", "base+" if exp["forward"] else "base-", label, bounded=False)
    finally:
        _set("gemm_tile", 0); _set("gemm_splitk", 0); _set("geglu_fwd", 1)
    del e64, e0


@pytest.mark.parametrize("dtype", D16)
@pytest.mark.parametrize("F", [64, 128, 192, 256])
def test_geglu_epilogues_under_every_tile_code(dtype, F, tmp_path, request):
    """rows = 77, (B, kps) = (2, 2), C = 72 under the twelve codes that fuse, 65 (64-column tile: unfused), 521 (fuses on its substitute 515) and the
    heuristic (K = 72: register-staged, unfused)"""
    acc, t0 = {}, time.time()
    for kind in ("G3", "G2"):
        _geglu_case(acc, kind, dtype, F, 72, 77, 2, 2, E.ALL_CODES, tmp_path)
    # the grid reaches both answers of the rule where the issue says so
    M = 308
    assert not E.geglu_fuses(dtype, 65, M, 2 * F, 72) and E.geglu_fuses(dtype, 515, M, 2 * F, 72) and not E.geglu_fuses(dtype, 0, M, 2 * F, 72)
    assert E.geglu_fuses(dtype, 518, M, 2 * F, 72) == E.geglu_fuses(dtype, 530, M, 2 * F, 72) == (F != 192 and F != 64)
    assert E.geglu_fuses(dtype, 515, M, F, 72) == (F in (128, 256)) and E.geglu_fuses(dtype, 518, M, F, 72) == (F == 256)
    _guard(acc, dtype, "geglu", request.node.name)
    print(f"\nepilogue ops: F={F} {NAME[dtype]}: {2 * len(E.ALL_CODES)} (net, code) pairs in {time.time() - t0:.1f} s")


EDGE_SHAPES = [(7, 2, 2, 72), (77, 1, 1, 72), (77, 1, 3, 72), (77, 2, 2, 64)]      # (rows, B, kps, C)


@pytest.mark.parametrize("dtype", D16)
@pytest.mark.parametrize("rows,B,kps,C", EDGE_SHAPES, ids=[f"rows{r}-B{b}k{k}-C{c}" for r, b, k, c in EDGE_SHAPES])
def test_geglu_epilogues_at_edge_shapes(dtype, rows, B, kps, C, tmp_path, request):
    """M below one 32-row slab, one sample with one / three tangents, exactly one K tile -- one code per distinct kernel body; F = 128 (the 256-column
    tiles fuse the tangent, not the adjoint) and F = 256 (everything fuses, two / four column tiles)"""
    acc = {}
    for F in (128, 256):
        for kind in ("G3", "G2"):
            _geglu_case(acc, kind, dtype, F, C, rows, B, kps, E.BODY_CODES, tmp_path)
    _guard(acc, dtype, "geglu", request.node.name)


@pytest.mark.parametrize("dtype", D16)
def test_geglu_heuristic_fuses_at_k_2048_and_not_at_72(dtype, tmp_path, request):
    """no forced code.  C = 2048 (K >= 2048: the BK = 64 ring 515), F = 128, rows = 77, (B, kps) = (1, 2): tangent and adjoint fuse; dpb_forward does
    not (its plain product, two tiles of K = 2048, splits four-fold).  The twin at C = 72 (register-staged kernel) fuses nothing."""
    assert E.geglu_expected("G3", dtype, 0, 128, 2048, 77, 1, 2) == {"primal": 0, "tangent": 1, "adjoint": 1, "forward": 0}
    assert E.geglu_expected("G2", dtype, 0, 128, 2048, 77, 1, 2) == {"primal": 0, "tangent": 1, "adjoint": 0, "forward": 0}
    assert not any(E.geglu_expected("G3", dtype, 0, 128, 72, 77, 1, 2).values())
    acc = {}
    for C in (2048, 72):
        for kind in ("G3", "G2"):
            _geglu_case(acc, kind, dtype, 128, C, 77, 1, 2, (0,), tmp_path)
    _guard(acc, dtype, "geglu", request.node.name)
    assert ("epi_geglu", "tangent", "fused") in acc and ("epi_geglu", "adjoint", "fused") in acc


def test_geglu_fp32_engine_never_fuses(tmp_path):
    """fp32 has no ring kernels: the interleaved net runs the plain product and the stand-alone GEGLU kernel under any code"""
    acc = {}
    for kind in ("G3", "G2"):
        _geglu_case(acc, kind, F32, 128, 72, 77, 2, 2, (0, 515), tmp_path)
    _guard(acc, F32, "geglu", "fp32")
    assert not any(arm == "fused" for _, _, arm in acc)


# =============================================================================================== LayerNorm
# (K, Cout, B, kps, ln_fuse values): rows = 77.  M = 308 / 154 fuse, M = 77 < 128 does not; K = 64 / 128 / 320 fuse the tangent, K = 72 does not;
# Cout = 64 fuses the adjoint, Cout = 72 (K of the adjoint product, no multiple of 64) does not, Cout = 1280 only under ln_fuse = 3
LN_CASES = ([(K, 64, B, kps, (1,)) for B, kps in ((2, 2), (1, 2), (1, 1)) for K in (64, 128, 320, 72)] +
            [(128, 1280, 2, 2, (1, 3)), (64, 72, 2, 2, (1,))])


def _ln_case(acc, kind, dtype, K, cout, B, kps, fuses, rows=77):
    steps = E.ln_net(kind, cout)
    params, x, V, U, ref = _prepared(f"{kind}co{cout}", steps, lambda g: E.ln_params(g, K, cout), K, cout + (E.LN_WIDTH if kind == "L3" else 0),
                                      rows, B, kps, dtype, 1.0)
    e = R.engine(R.build_tape(steps, params, dtype, DEV, rows, K), B, B * kps)
    label = f"{kind} K={K} Cout={cout} rows={rows} B={B} kps={kps}"
    try:
        _set("ln_fuse", 0)
        base = R.run_engine(e, x, V, U)
        for v in fuses:
            exp = E.ln_expected(dtype, v, K, cout, rows, B, kps)
            _set("ln_fuse", v)
            out = R.run_engine(e, x, V, U)
            for i, p in enumerate(PASSES):
                assert base[3][p] - out[3][p] == exp[p], (f"{label} {NAME[dtype]} ln_fuse={v} {p}: {out[3][p]} launches, {base[3][p]} under ln_fuse = 0; "
                                                          f"the rule expects {exp[p]} fewer (a silent route change)")
                _check(acc, out[i], ref[i], "epi_ln", dtype, p, "fused" if exp[p] else "unfused", f"{label} ln_fuse={v}")
                _check(acc, base[i], ref[i], "epi_ln", dtype, p, "base+" if exp[p] else "base-", f"{label} ln_fuse={v}", bounded=False)
    finally:
        _set("ln_fuse", 0)
    del e


@pytest.mark.parametrize("dtype", D16)
@pytest.mark.parametrize("kind", ["L1", "L2", "L3"])
def test_layernorm_epilogues(dtype, kind, request):
    acc = {}
    for K, cout, B, kps, fuses in LN_CASES:
        _ln_case(acc, kind, dtype, K, cout, B, kps, fuses)
    _guard(acc, dtype, "ln", request.node.name)
    assert ("epi_ln", "tangent", "fused") in acc and ("epi_ln", "adjoint", "fused") in acc and ("epi_ln", "adjoint", "unfused") in acc


def test_layernorm_fp32_engine_never_fuses():
    acc = {}
    for kind in ("L1", "L2", "L3"):
        _ln_case(acc, kind, F32, 128, 64, 2, 2, (1, 3))
    _guard(acc, F32, "ln", "fp32")
    assert not any(arm == "fused" for _, _, arm in acc)


# =============================================================================================== the family-wide guard
def test_fused_maxima_stay_within_1_25x_of_the_base_arm():
    """Over ALL the cases of a family (the figures of the docstring): the largest row and global error of the fused launches is at most 1.25 x the
    largest error of the base arm on the same cases -- the guard against having measured, and set the bounds from, a wrong kernel.  A row maximum is
    the extreme of a few hundred rows of one case, so it is judged over the whole family, once every test of the group has run in this session (a
    partial run checks the global figures, per test, only); prints the table of the docstring."""
    for (family, dtype, p, arm), m in sorted(_ACC.items(), key=str):
        print(f"EPI-MAX {family} {NAME[dtype]} {p} {arm} row={m[0]:.1e} glob={m[1]:.1e}")
    for (group, dtype), names in _DONE.items():
        if dtype == F32 or len(names) < TESTS_PER_DTYPE[group]:
            continue
        for (family, dt, p, arm), m in _ACC.items():
            if dt != dtype or arm != "fused" or family.startswith("epi_ln") != (group == "ln"):
                continue
            b = _ACC[(family, dt, p, "base+")]
            for what, f, u in (("row", m[0], b[0]), ("global", m[1], b[1])):
                assert f <= 1.25 * u, f"{family} {NAME[dt]} {p}: fused {what} maximum {f:.3e} > 1.25 x the base arm's {u:.3e} on the same cases"
