"""GroupNorm, LayerNorm, GEGLU, SiLU / GELU and concat at op level against an fp64 reference (tests/_norm_ref.py): tiny tapes on a fresh engine,
primal, tangent and adjoint, with B = 2, kps = 2 (a wrong j / kps mapping reads the wrong sample) and B = 1, kps = 1, and a proof of the route by
launch count (Engine.stats()[0]).

Route proof.  The launches of the norm are the launch count of the pass minus the count of the same tape with the norm swapped for an op of known
cost, plus that cost: SiLU (1 launch) for the primal pass; concat(x, x) (2 launches in every pass) for the tangent and adjoint passes, because the
engine's SiLU op is primal only (its derivative lives inside GroupNorm+SiLU).  GroupNorm: 1 (one-launch kernel), 2 (two passes, the apply pass adds
the block partials), 3 (two passes + gn_reduce_kernel); atomics statistics path: 3 primal (gn_finalize) / 2.  The expected route comes from the
rules of norm.hip restated in _norm_ref.gn_route, and every case also names the route it is there for.  LayerNorm is one launch on either kernel, so
the count cannot tell ln_rows_kernel from ln_kernel: LN_CASES states which kernel each width reaches per dtype, derived from ln_launch.  Slab cases:
lazy_reduce = 1 must launch exactly one kernel fewer than lazy_reduce = 0 in the pass whose norm takes the slabs.

Not reachable at op level, hence not tested: GEGLU with accumulate = 1 (the engine refuses a GEGLU input with a second consumer, because the primal
overwrites it in place) and tangent / adjoint of the SiLU / GELU ops (primal only).

Row error = |d row| / (|ref row| + 0.05 rms row norm of its tangent); a row is one (tangent, group) for GroupNorm outputs and cotangents, one token
row otherwise.  Every row of every output is compared.  Bounds (_norm_ref.BOUNDS) are twice the largest error measured on an MI355X over the cases of
a family.  Measured maxima, row / global, primal | tangent | adjoint:
    fp32 gn_fused    2.5e-07 / 9.0e-08 | 2.5e-07 / 1.1e-07 | 2.5e-07 / 1.1e-07
    bf16 gn_fused    2.0e-03 / 1.7e-03 | 1.8e-03 / 1.7e-03 | 2.0e-03 / 1.7e-03
    fp16 gn_fused    2.3e-04 / 2.1e-04 | 2.4e-04 / 2.1e-04 | 2.4e-04 / 2.1e-04
    fp32 gn_two_pass 4.1e-07 / 9.6e-08 | 3.8e-07 / 1.0e-07 | 3.8e-07 / 1.0e-07
    bf16 gn_two_pass 2.2e-03 / 1.7e-03 | 2.2e-03 / 1.8e-03 | 2.3e-03 / 1.7e-03
    fp16 gn_two_pass 2.6e-04 / 2.1e-04 | 2.8e-04 / 2.2e-04 | 2.8e-04 / 2.2e-04
    fp32 gn_atomic   2.0e-07 / 8.1e-08 | 2.0e-07 / 9.7e-08 | 1.7e-07 / 9.4e-08
    bf16 gn_atomic   1.9e-03 / 1.7e-03 | 2.0e-03 / 1.7e-03 | 2.1e-03 / 1.7e-03
    fp16 gn_atomic   2.4e-04 / 2.1e-04 | 2.5e-04 / 2.1e-04 | 2.4e-04 / 2.1e-04
    fp32 ln          1.4e-07 / 6.7e-08 | 1.9e-07 / 7.8e-08 | 1.6e-07 / 7.6e-08
    bf16 ln          2.3e-03 / 1.7e-03 | 2.3e-03 / 1.7e-03 | 2.4e-03 / 1.8e-03
    fp16 ln          2.7e-04 / 2.1e-04 | 2.9e-04 / 2.1e-04 | 2.8e-04 / 2.2e-04
    fp32 acc_gn      1.3e-07 / 7.8e-08 | 1.6e-07 / 9.2e-08 | 1.6e-07 / 9.5e-08
    bf16 acc_gn      1.9e-03 / 1.7e-03 | 1.9e-03 / 1.7e-03 | 2.4e-03 / 2.1e-03
    fp16 acc_gn      2.3e-04 / 2.1e-04 | 2.3e-04 / 2.1e-04 | 3.3e-04 / 2.6e-04
    fp32 acc_ln      1.4e-07 / 5.8e-08 | 1.6e-07 / 6.8e-08 | 1.6e-07 / 7.3e-08
    bf16 acc_ln      1.8e-03 / 1.7e-03 | 1.8e-03 / 1.7e-03 | 2.3e-03 / 2.1e-03
    fp16 acc_ln      2.2e-04 / 2.1e-04 | 2.4e-04 / 2.1e-04 | 3.2e-04 / 2.6e-04
    fp32 slab_gn     6.0e-07 / 4.6e-07 | 8.9e-07 / 6.4e-07 | 8.1e-07 / 6.4e-07
    bf16 slab_gn     3.4e-03 / 2.8e-03 | 4.0e-03 / 2.9e-03 | 4.0e-03 / 2.9e-03
    fp16 slab_gn     4.4e-04 / 3.5e-04 | 4.5e-04 / 3.7e-04 | 4.7e-04 / 3.7e-04
    fp32 slab_ln     3.8e-07 / 3.4e-07 | 4.9e-07 / 4.3e-07 | 4.8e-07 / 4.3e-07
    bf16 slab_ln     2.9e-03 / 2.7e-03 | 3.4e-03 / 2.9e-03 | 3.3e-03 / 2.9e-03
    fp16 slab_ln     3.6e-04 / 3.3e-04 | 4.2e-04 / 3.6e-04 | 4.7e-04 / 3.6e-04
    fp32 geglu       6.8e-08 / 3.6e-08 | 1.2e-07 / 5.7e-08 | 8.2e-08 / 4.6e-08
    bf16 geglu       2.4e-03 / 1.7e-03 | 3.8e-03 / 2.0e-03 | 3.6e-03 / 2.1e-03
    fp16 geglu       3.2e-04 / 2.2e-04 | 4.8e-04 / 2.6e-04 | 4.7e-04 / 3.2e-04
    fp32 unary       8.2e-08 / 4.7e-08
    bf16 unary       2.2e-03 / 1.5e-03
    fp16 unary       2.8e-04 / 1.9e-04
    fp32 concat      1.3e-07 / 7.4e-08 | 2.2e-07 / 9.8e-08 | 2.1e-07 / 1.0e-07
    bf16 concat      4.4e-03 / 2.1e-03 | 4.9e-03 / 2.5e-03 | 6.0e-03 / 2.6e-03
    fp16 concat      3.8e-04 / 2.5e-04 | 7.8e-04 / 3.1e-04 | 8.1e-04 / 3.2e-04

Offset ladder (groups / rows with mean +-m and spread s; primal and tangent, which reads rstd and xhat): the engine's largest row error must be at
most 8x that of torch.nn.functional.group_norm / layer_norm in the same dtype on the same device and inputs.
  kernel route dtype pass mean/std: engine before the shifted statistics -> engine now | torch   (n/r: not reached, the run stopped at the first failing rung)
    gn fused  fp32 tangent 0/1: 7.4e-08 -> 8.0e-08 | 1.0e-07
    gn fused  fp32 primal  8/1: 2.4e-06 -> 5.0e-07 | 5.9e-07
    gn fused  fp32 tangent 8/1: 2.5e-06 -> 1.2e-07 | 1.2e-07
    gn fused  fp32 primal  64/0.25: n/r -> 1.2e-05 | 2.6e-05
    gn fused  fp32 tangent 64/0.25: n/r -> 9.1e-07 | 2.3e-06
    gn fused  fp32 primal  256/0.25: n/r -> 6.0e-05 | 9.7e-05
    gn fused  fp32 tangent 256/0.25: n/r -> 5.8e-06 | 7.3e-06
    gn fused  fp16 primal  64/0.25: 2.7e-03 -> 2.2e-04 | 8.7e-02
    gn fused  fp16 tangent 64/0.25: 2.9e-03 -> 2.3e-04 | 8.0e-03
    gn red    fp32 tangent 0/1: 7.0e-08 -> 7.0e-08 | 1.2e-07
    gn red    fp32 primal  8/1: 1.2e-06 -> 3.7e-07 | 5.5e-07
    gn red    fp32 tangent 8/1: 1.3e-06 -> 8.7e-08 | 9.0e-08
    gn red    fp32 primal  64/0.25: n/r -> 1.3e-05 | 2.4e-05
    gn red    fp32 tangent 64/0.25: n/r -> 4.3e-07 | 9.7e-07
    gn red    fp32 primal  256/0.25: n/r -> 5.1e-05 | 8.3e-05
    gn red    fp32 tangent 256/0.25: n/r -> 1.4e-06 | 3.5e-06
    gn red    fp16 primal  64/0.25: 1.0e-03 -> 2.1e-04 | 3.6e-02
    gn red    fp16 tangent 64/0.25: 1.0e-03 -> 2.1e-04 | 1.4e-03
    gn reduce fp32 tangent 0/1: 6.9e-08 -> 8.6e-08 | 9.3e-08
    gn reduce fp32 primal  8/1: 5.3e-07 -> 3.9e-07 | 8.8e-07
    gn reduce fp32 tangent 8/1: 4.6e-07 -> 7.2e-08 | 9.3e-08
    gn reduce fp32 primal  64/0.25: 3.8e-04 -> 1.1e-05 | 2.0e-05
    gn reduce fp32 tangent 64/0.25: n/r -> 5.8e-07 | 1.4e-06
    gn reduce fp32 primal  256/0.25: n/r -> 5.3e-05 | 8.0e-05
    gn reduce fp32 tangent 256/0.25: n/r -> 2.1e-06 | 3.4e-06
    gn reduce fp16 primal  64/0.25: 1.0e-03 -> 2.6e-04 | 6.1e-02
    gn reduce fp16 tangent 64/0.25: 1.0e-03 -> 2.1e-04 | 2.1e-03
    ln rows   fp32 primal  64/0.25: 3.4e-05 -> 3.4e-05 | 2.9e-05
    ln rows   fp32 tangent 64/0.25: 4.9e-06 -> 4.9e-06 | 3.3e-06
    ln rows   fp32 primal  256/0.25: 1.3e-04 -> 1.3e-04 | 1.4e-04
    ln rows   fp32 tangent 256/0.25: 1.4e-05 -> 1.4e-05 | 1.3e-05
    ln rows   fp16 primal  64/0.25: 2.2e-04 -> 2.2e-04 | 3.4e-04
    ln rows   fp16 tangent 64/0.25: 2.4e-04 -> 2.4e-04 | 3.6e-04
    ln wave   fp32 primal  64/0.25: 2.6e-05 -> 2.6e-05 | 2.2e-05
    ln wave   fp32 tangent 64/0.25: 1.9e-06 -> 1.9e-06 | 2.8e-06
    ln wave   fp32 primal  256/0.25: 9.3e-05 -> 9.3e-05 | 1.1e-04
    ln wave   fp32 tangent 256/0.25: 7.9e-06 -> 7.9e-06 | 1.1e-05
    ln wave   fp16 primal  64/0.25: 2.2e-04 -> 2.2e-04 | 3.1e-04
    ln wave   fp16 tangent 64/0.25: 2.3e-04 -> 2.3e-04 | 3.5e-04
"""

import math

import pytest
import torch

import _norm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DT = [pytest.param(F32, id="fp32"), pytest.param(BF, id="bf16"), pytest.param(F16, id="fp16")]
D16 = [pytest.param(BF, id="bf16"), pytest.param(F16, id="fp16")]
NAME = {F32: "fp32", BF: "bf16", F16: "fp16"}
BK = ((2, 2), (1, 1))                                   # (B, kps)
PASSES = ("primal", "tangent", "adjoint")


def _lib():
    from diffusion_pullback_amd import lib as L
    return L.load()


def _set(key: str, value: int):
    from diffusion_pullback_amd import lib as L
    L.check(_lib().dpb_debug_set(key.encode(), value))


_BASE = {}


def _swap(steps, names, repl):
    out = []
    for s in steps:
        if s["op"] in ("gn", "ln") and s["name"] in names:
            out.append(R.unary(s["out"], s["src"], "silu") if repl == "silu" else R.concat(s["out"], s["src"], s["src"]))
        else:
            out.append(s)
    return out


def _baseline(steps, names, dtype, B, kps):
    """launch counts per pass of the same tape with the norms `names` swapped for SiLU (primal) / concat(x, x) (tangent, adjoint), on a small
    shape (launch counts of these ops do not depend on it); cached"""
    key = (tuple((s["op"], s["out"], s["src"], s.get("src2")) for s in steps), tuple(names), dtype, B, kps)
    if key not in _BASE:
        rows, C = 8, 64
        g = torch.Generator().manual_seed(1)
        x = R.plain_input(g, (B, rows, C), dtype).to(DEV)
        nt = B * kps
        e = R.engine(R.build_tape(_swap(steps, names, "silu"), {}, dtype, DEV, rows, C), B, nt)
        n = {"primal": R.run_engine(e, x, None, None)[3]["primal"]}
        del e
        sw = _swap(steps, names, "concat")
        widths = {"x": C}
        for s in sw:
            widths[s["out"]] = widths[s["src"]] + widths[s["src2"]] if s["op"] == "concat" else widths[s["src"]]
        Cout = widths[sw[-1]["out"]]
        e = R.engine(R.build_tape(sw, {}, dtype, DEV, rows, C), B, nt)
        _, _, _, m = R.run_engine(e, x, R.plain_input(g, (nt, rows, C), dtype).to(DEV), R.plain_input(g, (nt, rows, Cout), dtype).to(DEV))
        n["tangent"], n["adjoint"] = m["tangent"], m["adjoint"]
        del e
        _BASE[key] = n
    return _BASE[key]


def run_net(steps, params, dtype, rows, C, B, kps, family, groups_out, groups_in, seed, label, launches=None, norms=(), scale=1.0, x=None,
            passes=PASSES, bounds=True):
    """One net on a fresh engine against the fp64 reference.  launches: {pass: launches the norms `norms` must account for}.  groups_out / groups_in:
    the comparator's groups for the output (primal, tangent) and the input cotangent.  Returns ({pass: (row, glob)}, outputs, launch counts)."""
    g = torch.Generator().manual_seed(seed)
    nt = B * kps
    if x is None:
        x = R.plain_input(g, (B, rows, C), dtype, scale)
    tape = R.build_tape(steps, params, dtype, DEV, rows, C)
    Cout = tape.buffers[tape.taps["o"]][1]
    V = R.plain_input(g, (nt, rows, C), dtype).to(DEV) if "tangent" in passes else None
    U = R.plain_input(g, (nt, rows, Cout), dtype).to(DEV) if "adjoint" in passes else None
    xd = x.to(DEV)
    e = R.engine(tape, B, nt)
    O, dO, gX, n = R.run_engine(e, xd, V, U)
    del e
    ref = R.reference(steps, params, xd, dtype, V, U, kps)
    if launches is not None:
        base = _baseline(steps, norms, dtype, B, kps)
        for p in passes:
            seen = n[p] - base[p] + len(norms) * (1 if p == "primal" else 2)
            assert seen == launches[p], f"{label} {p}: the norm took {seen} launches, expected {launches[p]} (a silent route change)"
    got = {}
    for p, out, r, grp in (("primal", O, ref[0], groups_out), ("tangent", dO, ref[1], groups_out), ("adjoint", gX, ref[2], groups_in)):
        if p not in passes:
            continue
        rb, gb = R.bound(family, dtype, p) if bounds else (math.inf, math.inf)
        row, glob = R.errors(out, r, grp)
        print(f"NORM-ERR {family} {NAME[dtype]} {p} {label} B={B} kps={kps} row={row:.3e} glob={glob:.3e}")
        R.compare(out, r, grp, rb, gb, f"{p} {family} {NAME[dtype]} {label} B={B} kps={kps}")
        got[p] = (row, glob)
    return got, (O, dO, gX), n


# =============================================================================================== GroupNorm
# (C, HW, the route the case is there for: 16-bit, fp32 -- per primal pass of one sample)
GN_CASES = [
    (320, 64, "fused", "fused"),
    (320, 100, "fused", "fused"),          # ragged against the 102 pixels per sweep
    (320, 408, "fused", "fused"),          # the last fused size
    (1920, 136, "fused", "fused"),         # 16 bit: two groups per window, 15 chunk columns
    (2560, 204, "fused", "red"),           # fp32: 20 chunk columns per group do not fit the window: two passes, ncp = 3
    (256, 512, "fused", "fused"),
    (320, 409, "red", "red"),              # just past the fused limit
    (2560, 205, "red", "red"),             # ncp = 2 (16 bit) / 3 (fp32)
    (32, 72, "red", "red"),                # cpg = 1 < CH: per-channel branch
    (128, 72, "red", "fused"),             # 16 bit: cpg = 4 < CH = 8 (the autoencoder's width, never fused there); fp32 fuses (cpg = CH)
]


def _gn_case(dtype, C, HW, silu, B, kps, seed, family=None, det=True, want=None):
    G = 32
    g = torch.Generator().manual_seed(seed)
    params = R.norm_params(g, ["n"], C)
    steps = [R.gn("o", "x", "n", G, 1e-5, silu)]
    nt = B * kps
    exp, routes = {}, {}
    for p in PASSES:
        routes[p], exp[p] = R.gn_route(C, G, HW, dtype, B if p == "primal" else nt, det, p == "primal")
    if want is not None:
        assert routes["primal"] == want, (C, HW, dtype, routes, want)
    # one engine for the three passes; the family of a pass follows its route
    fams = {p: family or ("gn_fused" if routes[p] == "fused" else "gn_atomic" if routes[p] == "atomic" else "gn_two_pass") for p in PASSES}
    return _gn_run(steps, params, dtype, HW, C, B, kps, fams, G, seed, f"C={C} HW={HW} silu={int(silu)} {'/'.join(routes[p] for p in PASSES)}", exp)


def _gn_run(steps, params, dtype, rows, C, B, kps, fams, G, seed, label, exp):
    g = torch.Generator().manual_seed(seed + 1000)
    nt = B * kps
    x = R.plain_input(g, (B, rows, C), dtype).to(DEV)
    V = R.plain_input(g, (nt, rows, C), dtype).to(DEV)
    U = R.plain_input(g, (nt, rows, C), dtype).to(DEV)
    e = R.engine(R.build_tape(steps, params, dtype, DEV, rows, C), B, nt)
    O, dO, gX, n = R.run_engine(e, x, V, U)
    del e
    ref = R.reference(steps, params, x, dtype, V, U, kps)
    base = _baseline(steps, ("n",), dtype, B, kps)
    for p, out, r in (("primal", O, ref[0]), ("tangent", dO, ref[1]), ("adjoint", gX, ref[2])):
        seen = n[p] - base[p] + (1 if p == "primal" else 2)
        assert seen == exp[p], f"{label} {p}: GroupNorm took {seen} launches, expected {exp[p]} (a silent route change)"
        rb, gb = R.bound(fams[p], dtype, p)
        row, glob = R.errors(out, r, G)
        print(f"NORM-ERR {fams[p]} {NAME[dtype]} {p} {label} B={B} kps={kps} row={row:.3e} glob={glob:.3e}")
        R.compare(out, r, G, rb, gb, f"{p} {fams[p]} {NAME[dtype]} {label} B={B} kps={kps}")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("C,HW,r16,r32", GN_CASES, ids=[f"C{c}-HW{hw}" for c, hw, _, _ in GN_CASES])
def test_groupnorm_routes(dtype, C, HW, r16, r32):
    for silu in (False, True):
        for B, kps in BK:
            _gn_case(dtype, C, HW, silu, B, kps, seed=C + HW + int(silu), want=(r32 if dtype == F32 else r16) if B == 1 else None)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("HW,want", [(2048, "red"), (2056, "reduce")], ids=["256blocks", "257blocks"])
def test_groupnorm_block_count_threshold(dtype, HW, want):
    """C = 32, one sample / tangent: ppb = 8, HW = 2048 -> 256 statistics blocks (the apply pass reduces), 2056 -> 257 (gn_reduce_kernel); with four
    tangents the rule picks larger blocks and the tangent / adjoint passes of both sizes reduce in the apply pass"""
    for silu in (False, True):
        _gn_case(dtype, 32, HW, silu, 1, 1, seed=HW + int(silu), want=want)
        _gn_case(dtype, 32, HW, silu, 2, 2, seed=HW + 7 + int(silu))
    assert R.gn_route(32, 32, HW, dtype, 4)[0] == "red" and R.gn_route(32, 32, HW, dtype, 2)[0] == want


@pytest.mark.parametrize("dtype", DT)
def test_groupnorm_atomics_statistics_path(dtype):
    """gn_deterministic = 0: LDS float atomics + one fp64 global atomic per group per block, run-time ordered (one shape per two-pass route; the
    one-launch kernel has no atomics and is checked to stay on its route)"""
    try:
        _set("gn_deterministic", 0)
        for C, HW in ((320, 409), (32, 2056), (128, 72) if dtype != F32 else (32, 72)):
            for silu in (False, True):
                for B, kps in BK:
                    _gn_case(dtype, C, HW, silu, B, kps, seed=C + HW, det=False, want="atomic" if B == 1 else None)
        _gn_case(dtype, 320, 64, True, 2, 2, seed=5, det=False)
    finally:
        _set("gn_deterministic", 1)


# =============================================================================================== LayerNorm
# C -> the kernel ln_launch picks (nch = C / CH chunks per row, CH = 8 / 4; ln_rows_kernel<LPR, NI> when nch = LPR x {3, 5}, LPR = 8, 16, 32 tried in
# that order; else ln_kernel<MAXI>, need = ceil(nch / 64), need = 4 runs on MAXI = 5):
#   16 bit: 192 rows8x3, 320 rows8x5, 640 rows16x5, 768 rows32x3, 1280 rows32x5; 64 wave1, 512 wave1, 1024 wave2, 1536 wave3, 2048 wave5 (need 4),
#           2560 wave5; 384 rows16x3
#   fp32:   96 rows8x3, 160 rows8x5, 192 rows16x3, 320 rows16x5, 384 rows32x3, 640 rows32x5; 768 wave3, 1280 wave5, 64 wave1, 512 wave2, 1024 wave5 (need 4)
#           (1536, 2048 and 2560 exceed the 320 chunks a row may have in fp32)
LN_CASES = {
    16: {192: "rows8x3", 320: "rows8x5", 384: "rows16x3", 640: "rows16x5", 768: "rows32x3", 1280: "rows32x5",
         64: "wave1", 512: "wave1", 1024: "wave2", 1536: "wave3", 2048: "wave5", 2560: "wave5"},
    32: {96: "rows8x3", 160: "rows8x5", 192: "rows16x3", 320: "rows16x5", 384: "rows32x3", 640: "rows32x5",
         768: "wave3", 1280: "wave5", 64: "wave1", 512: "wave2", 1024: "wave5"},
}


@pytest.mark.parametrize("dtype", DT)
def test_layernorm_kernels_and_ragged_rows(dtype):
    """row counts 77 and 7 are ragged against every rows-per-block value (4 waves x 64 / LPR rows = 32, 16, 8; 4 for ln_kernel); 64 is a multiple"""
    cases = LN_CASES[32 if dtype == F32 else 16]
    assert {v for v in cases.values()} >= {"rows8x3", "rows8x5", "rows16x3", "rows16x5", "rows32x3", "rows32x5", "wave1", "wave2", "wave3", "wave5"}
    for C, kernel in cases.items():
        assert R.ln_route(C, dtype) == kernel, (C, dtype, R.ln_route(C, dtype), kernel)
        g = torch.Generator().manual_seed(C)
        params = R.norm_params(g, ["n"], C)
        steps = [R.ln("o", "x", "n")]
        for rows in (77, 7, 64):
            for B, kps in BK if rows != 64 else ((2, 2),):
                run_net(steps, params, dtype, rows, C, B, kps, "ln", 0, 0, C + rows, f"C={C} rows={rows} {kernel}",
                        launches={p: 1 for p in PASSES}, norms=("n",))


# =============================================================================================== accumulate: two consumers of x
@pytest.mark.parametrize("dtype", DT)
def test_two_consumers_accumulate_into_one_cotangent(dtype):
    """x feeds two norms with different gamma, the concat of the two outputs is the tap: the second adjoint to arrive runs with accumulate = 1"""
    for kind, C, rows_list in (("gn", 320, (64, 409)), ("gn", 32, (2056,)), ("ln", 320, (77,)), ("ln", 512, (77,))):
        g = torch.Generator().manual_seed(C)
        params = R.norm_params(g, ["n", "m"], C)
        mk = (lambda o, n: R.gn(o, "x", n, 32, 1e-5, True)) if kind == "gn" else (lambda o, n: R.ln(o, "x", n))
        steps = [mk("a", "n"), mk("b", "m"), R.concat("o", "a", "b")]
        for rows in rows_list:
            for B, kps in BK:
                if kind == "gn":
                    nl = {p: 2 * R.gn_route(C, 32, rows, dtype, B if p == "primal" else B * kps)[1] for p in PASSES}
                    fam = "acc_gn"
                else:
                    nl = {p: 2 for p in PASSES}
                    fam = "acc_ln"
                run_net(steps, params, dtype, rows, C, B, kps, fam, 64 if kind == "gn" else 0, 32 if kind == "gn" else 0, C + rows,
                        f"{kind} x2 C={C} rows={rows}", launches=nl, norms=("n", "m"))


# =============================================================================================== split-K slabs handed to the norm (SlabSrc)
def _linear_params(g, name, cout, cin, bias=True):
    p = {name + ".weight": torch.randn(cout, cin, generator=g) / math.sqrt(cin)}
    if bias:
        p[name + ".bias"] = 0.5 * torch.randn(cout, generator=g)
    return p


def _slab_nets(kind, K, C):
    """product K -> C, norm, product C -> K: the tangent of the first product and the adjoint of the second leave their slabs to the norm"""
    norm = R.gn("z", "h", "n", 32, 1e-5, True) if kind == "gn" else R.ln("z", "h", "n")
    return [R.linear("h", "x", "p1", C), norm, R.linear("o", "z", "p2", K)]


def _slab_case(dtype, steps, params, rows, K, splitk, B, kps, family, label, expect_fewer, seed=0):
    """runs the net with lazy_reduce 1 and 0 under a forced split; both against the fp64 reference; returns the two outputs"""
    g = torch.Generator().manual_seed(seed)
    nt = B * kps
    x = R.plain_input(g, (B, rows, K), dtype).to(DEV)
    tape = R.build_tape(steps, params, dtype, DEV, rows, K)
    Cout = tape.buffers[tape.taps["o"]][1]
    V = R.plain_input(g, (nt, rows, K), dtype).to(DEV)
    U = R.plain_input(g, (nt, rows, Cout), dtype).to(DEV)
    ref = R.reference(steps, params, x, dtype, V, U, kps)
    e = R.engine(tape, B, nt)
    outs, counts = {}, {}
    try:
        _set("gemm_tile", 64); _set("gemm_splitk", splitk)
        for lazy in (1, 0):
            _set("lazy_reduce", lazy)
            O, dO, gX, n = R.run_engine(e, x, V, U)
            outs[lazy], counts[lazy] = (O.clone(), dO.clone(), gX.clone()), n
    finally:
        _set("lazy_reduce", 1); _set("gemm_tile", 0); _set("gemm_splitk", 0)
    del e
    for lazy in (1, 0):
        for p, out, r in zip(PASSES, outs[lazy], ref):
            rb, gb = R.bound(family, dtype, p)
            row, glob = R.errors(out, r, 0)
            print(f"NORM-ERR {family} {NAME[dtype]} {p} {label} splitk={splitk} lazy={lazy} B={B} kps={kps} row={row:.3e} glob={glob:.3e}")
            R.compare(out, r, 0, rb, gb, f"{p} {family} {NAME[dtype]} {label} splitk={splitk} lazy={lazy}")
    for p in PASSES:
        fewer = counts[0][p] - counts[1][p]
        assert fewer == expect_fewer[p], (f"{label} splitk={splitk} {p}: lazy_reduce=1 launched {counts[1][p]} kernels, lazy_reduce=0 {counts[0][p]}; "
                                          f"expected {expect_fewer[p]} fewer (a silent route change)")
    for a, b in zip(outs[1], outs[0]):
        assert torch.equal(a, b), f"{label} splitk={splitk}: the deferred reduction is not bitwise the separate reduce kernel"


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("splitk", [3, 4, 8, 13])
def test_groupnorm_takes_split_k_slabs(dtype, splitk):
    """K = 2560 -> C = 320, HW = 64 (one-launch GroupNorm), splits 3 (scalar arm of slab_chunk), 4 (4-wide), 8 (8-wide), 13 (8 + 4 + 1)"""
    g = torch.Generator().manual_seed(splitk)
    params = {**R.norm_params(g, ["n"], 320), **_linear_params(g, "p1", 320, 2560), **_linear_params(g, "p2", 2560, 320)}
    _slab_case(dtype, _slab_nets("gn", 2560, 320), params, 64, 2560, splitk, 2, 2, "slab_gn", "gn K=2560->320 HW=64",
               {"primal": 0, "tangent": 1, "adjoint": 1}, seed=splitk)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("splitk", [3, 4, 8, 13])
def test_layernorm_takes_split_k_slabs(dtype, splitk):
    """K = 1280 -> C = 320, 64 rows; B = 1, kps = 3: 192 tangent rows"""
    g = torch.Generator().manual_seed(splitk)
    params = {**R.norm_params(g, ["n"], 320), **_linear_params(g, "p1", 320, 1280), **_linear_params(g, "p2", 1280, 320)}
    _slab_case(dtype, _slab_nets("ln", 1280, 320), params, 64, 1280, splitk, 1, 3, "slab_ln", "ln K=1280->320 rows=64",
               {"primal": 0, "tangent": 1, "adjoint": 1}, seed=splitk)


@pytest.mark.parametrize("dtype", DT)
def test_layernorm_slab_with_a_second_reader_stores_the_reduced_tensor(dtype):
    """h = product(x); o = concat(LayerNorm(h), h): the concat reads h too, so the LayerNorm tangent that adds the slabs also writes h (SlabSrc::store);
    77 rows: ragged against ln_rows_kernel's 8 rows per wave (dead row groups load no slab).  The adjoint has no slab (the LayerNorm accumulates
    onto the concat's cotangent of h)."""
    g = torch.Generator().manual_seed(3)
    params = {**R.norm_params(g, ["n"], 320), **_linear_params(g, "p1", 320, 1280)}
    steps = [R.linear("h", "x", "p1", 320), R.ln("z", "h", "n"), R.concat("o", "z", "h")]
    for splitk in (4, 13):
        _slab_case(dtype, steps, params, 77, 1280, splitk, 2, 2, "slab_ln", "ln+store K=1280->320 rows=77", {"primal": 0, "tangent": 1, "adjoint": 0}, seed=splitk)


@pytest.mark.parametrize("dtype", DT)
def test_groupnorm_slab_with_residual(dtype):
    """c = product_b(x) + product_a(x); GroupNorm(c): the deferred reduction adds the residual's tangent (SlabSrc::R) before it rounds"""
    g = torch.Generator().manual_seed(4)
    params = {**R.norm_params(g, ["n"], 320), **_linear_params(g, "pa", 320, 2560), **_linear_params(g, "pb", 320, 2560)}
    steps = [R.linear("r", "x", "pa", 320), R.linear("c", "x", "pb", 320, res="r"), R.gn("o", "c", "n", 32, 1e-5, True)]
    for splitk in (3, 8):
        _slab_case(dtype, steps, params, 64, 2560, splitk, 2, 2, "slab_gn", "gn+res K=2560->320 HW=64", {"primal": 0, "tangent": 1, "adjoint": 0}, seed=splitk)


# =============================================================================================== GEGLU, SiLU / GELU, concat
@pytest.mark.parametrize("dtype", DT)
def test_geglu_layouts_stash_and_passes(dtype):
    """inputs scaled by 4: the gate covers both GELU tails.  primal() stashes the factors (G1, G2) over its input; forward() does not and must give
    the same output bits"""
    for F, il in ((64, 0), (64, 64), (1280, 0), (1280, 64), (320, 0)):
        steps = [R.geglu("o", "x", il)]
        for rows in (77, 7):
            for B, kps in BK:
                _, (O, _, _), n = run_net(steps, {}, dtype, rows, 2 * F, B, kps, "geglu", 0, 0, F + rows + il, f"F={F} il={il} rows={rows}", scale=4.0)
                g = torch.Generator().manual_seed(F + rows + il)
                x = R.plain_input(g, (B, rows, 2 * F), dtype, 4.0).to(DEV)
                e = R.engine(R.build_tape(steps, {}, dtype, DEV, rows, 2 * F), B, B * kps)
                Of, _, _, nf = R.run_engine(e, x, None, None, forward_only=True)
                del e
                assert torch.equal(Of, O), f"GEGLU F={F} il={il}: forward (no stash) and primal (stash) outputs differ"
                assert nf["primal"] == n["primal"]


@pytest.mark.parametrize("dtype", DT)
def test_silu_quick_gelu_gelu_primal(dtype):
    """77 x 40: 385 (16 bit) / 770 (fp32) chunks, ragged against the 256 threads of a block; these ops are primal only in the engine"""
    for fn in ("silu", "quick_gelu", "gelu"):
        for B in (2, 1):
            run_net([R.unary("o", "x", fn)], {}, dtype, 77, 40, B, 1, "unary", 0, 0, 40 + B, fn, scale=3.0, passes=("primal",))


@pytest.mark.parametrize("dtype", DT)
def test_concat_splits_the_tangent_and_routes_the_adjoint(dtype):
    """o = concat(LayerNorm_a(x) [48], GEGLU(LayerNorm_b(x)) [24]): Ca != Cb, both multiples of 8; the adjoint sends each column window to its input"""
    g = torch.Generator().manual_seed(9)
    params = R.norm_params(g, ["n", "m"], 48)
    steps = [R.ln("a", "x", "n"), R.ln("b0", "x", "m"), R.geglu("b", "b0"), R.concat("o", "a", "b")]
    for B, kps in BK:
        run_net(steps, params, dtype, 77, 48, B, kps, "concat", 0, 0, 11, "concat 48+24")


# =============================================================================================== offset ladder
def _torch_norm(kind, x, V, gamma, beta, G, dtype, kps):
    """torch.nn.functional.group_norm / layer_norm in the engine dtype (fp32 engine: fp32) on x [B, rows, C]: output and forward-mode tangent"""
    F = torch.nn.functional
    xt = x.to(dtype)
    ga, be = gamma.to(DEV, dtype), beta.to(DEV, dtype)
    if kind == "gn":
        f = lambda a: F.group_norm(a.permute(0, 2, 1), G, ga, be, 1e-5).permute(0, 2, 1)
    else:
        f = lambda a: F.layer_norm(a, (a.shape[-1],), ga, be, 1e-5)
    idx = torch.arange(V.shape[0], device=x.device) // kps
    O = f(xt)
    _, dO = torch.func.jvp(f, (xt[idx],), (V.to(dtype),))
    return O.float(), dO.float()


LADDER_CASES = [("gn", 320, 64, "fused"), ("gn", 320, 409, "red"), ("gn", 32, 2056, "reduce"), ("ln", 320, 77, "rows"), ("ln", 512, 77, "wave")]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("kind,C,rows,route", LADDER_CASES, ids=[f"{k}-{r}" for k, _, _, r in LADDER_CASES])
def test_offset_ladder_against_torch(dtype, kind, C, rows, route):
    """groups (GroupNorm) or rows (LayerNorm) whose mean is large against their spread: the engine may be at most 8x worse than torch's own kernel
    in the same dtype (the margin allows for another fp32 summation order; real cancellation costs orders of magnitude)"""
    G = 32 if kind == "gn" else 0
    B, kps = 1, 2
    if kind == "gn":
        assert R.gn_route(C, G, rows, dtype, 1)[0] == route
    else:
        assert R.ln_route(C, dtype).startswith(route)
    for m, s in R.ladder_rungs(dtype):
        g = torch.Generator().manual_seed(int(m) + C)
        gamma, beta = R.affine(g, C)
        params = {"n.weight": gamma, "n.bias": beta}
        steps = [R.gn("o", "x", "n", G, 1e-5, False) if kind == "gn" else R.ln("o", "x", "n")]
        x = R.ladder_input(g, B, rows, C, dtype, m, s, G).to(DEV)
        V = R.plain_input(g, (B * kps, rows, C), dtype).to(DEV)
        e = R.engine(R.build_tape(steps, params, dtype, DEV, rows, C), B, B * kps)
        O, dO, _, _ = R.run_engine(e, x, V, None)
        del e
        ref = R.reference(steps, params, x, dtype, V, None, kps)
        tO, tdO = _torch_norm(kind, x, V, gamma, beta, G, dtype, kps)
        for p, out, tout, r in (("primal", O, tO, ref[0]), ("tangent", dO, tdO, ref[1])):
            assert torch.isfinite(out).all()
            mine, theirs = R.errors(out, r, G)[0], R.errors(tout, r, G)[0]
            print(f"LADDER {kind} {route} {NAME[dtype]} {p} mean={m:g} std={s:g} engine={mine:.3e} torch={theirs:.3e} ratio={mine / theirs:.2f}")
            assert mine <= 8 * theirs, (f"{kind} {route} {NAME[dtype]} {p} at mean {m:g} / std {s:g}: engine row error {mine:.3e} > 8 x torch's "
                                        f"{theirs:.3e}")
