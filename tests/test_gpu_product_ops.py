"""Every conv / linear product route (OP_CONV behind the tile table kGemmTiles, csrc/kernels.h) against an exact fp64 reference at op level: tiny
tapes of one or two Tape.conv ops (tests/_product_ref.py), primal, tangent and adjoint, under every forced tile code, the heuristic, and the split
counts heuristic / 1 / 3, in bf16, fp16 and (register-staged tiles) fp32.  tests/test_gpu_gemm_tiles.py and the *_bitwise_equals_* tests compare the
kernels with the BK = 64 ring (code 515) or a sibling loop; this file pins 515 itself, and what all the kernels share.

Two tiers per case (derivations in tests/_product_ref.py):
  exact  small-integer data: the engine's output must equal ref64.float().to(dtype) bit for bit in every element (torch.equal, no tolerance);
  real   Gaussian data rounded to the engine dtype: every element within u_T (|ref| + E) + E, E = 2 (K_total + 4) 2^-24 S (+ the stated terms for
         intermediates stored in the engine dtype).
Route proof: with profiling on, every product's bracket (`big` column of the dump) is the kind include/dpb.h documents for the forced code, or the
kind of the code's documented substitute row (515, kind 4) where the tile does not take the product -- the rule of pick_async_tile restated in
`_expected_kind`; code 600 on a product the halo kernel does not take leaves the heuristic in charge, as documented.  A forced split is proven by
the launch count: one launch more than the unsplit pass per product that the clamp of gemm_plan leaves split.

Measured on an MI355X (a record, not the bound): every exact-tier comparison is torch.equal; the largest real-tier |got - ref| / bound per
(family, dtype) as primal / tangent / adjoint:
  reg          fp32 0.103 / 0.084 / 0.047    bf16 0.992 / 0.985 / 0.988    fp16 0.957 / 0.971 / 0.959
  ring32       bf16 0.992 / 0.985 / 0.988    fp16 0.957 / 0.971 / 0.959
  ring64       bf16 0.992 / 0.985 / 0.988    fp16 0.957 / 0.971 / 0.959
  ring64-half  bf16 0.992 / 0.985 / 0.988    fp16 0.957 / 0.971 / 0.959
  p8           bf16 0.992 / 0.985 / 0.988    fp16 0.957 / 0.971 / 0.959
  wres         bf16 0.981 / 0.985 / 0.970    fp16 0.942 / 0.971 / 0.959
  halo         bf16 0.992 / 0.985 / 0.988    fp16 0.957 / 0.960 / 0.954
  heuristic    fp32 0.103 / 0.084 / 0.047    bf16 0.992 / 0.985 / 0.988    fp16 0.957 / 0.971 / 0.959
(16-bit: the one rounding of an element that sits just below a rounding boundary -- the bound has no room for a second rounding; the families agree
because each maximum is such an element of a case they share, which every kernel rounds alike.  fp32: the accumulation error, a tenth of E.)
The file: 18 tests in about 7 s, the longest 1.6 s (the first, which loads the library).  No kernel or tape bug was found.
"""
import csv
import time
import zlib

import pytest
import torch

import _product_ref as R

pytestmark = pytest.mark.gpu

BF, F16, F32 = R.BF, R.F16, R.F32
# forced code -> (family, profile kind, gathers its kernel is built for: n plain rows / c forward + transposed gather / u upsampling gather,
#                 gathers whole 64-channel K tiles only) -- the forceable rows of kGemmTiles; kinds as include/dpb.h documents them
CODES = {
    64: ("reg", 0, "ncu", False), 128: ("reg", 1, "ncu", False),
    129: ("ring32", 2, "ncu", False), 131: ("ring32", 2, "ncu", False), 133: ("ring32", 2, "ncu", False), 257: ("ring32", 2, "ncu", False),
    65: ("ring32", 3, "ncu", False), 67: ("ring32", 3, "ncu", False),
    512: ("ring64", 4, "ncu", False), 513: ("ring64", 4, "ncu", False), 514: ("ring64", 4, "ncu", False), 515: ("ring64", 4, "ncu", False),
    516: ("ring64", 4, "ncu", False), 517: ("ring64", 4, "ncu", False), 518: ("ring64", 6, "n", False),
    521: ("ring64-half", 4, "nc", False), 522: ("ring64-half", 4, "n", False), 523: ("ring64-half", 4, "n", False),
    530: ("p8", 11, "ncu", True), 540: ("wres", 12, "n", False), 600: ("halo", 5, "c", True),
}
SUBSTITUTE_KIND = 4                                   # every row that has a substitute names 515 (T_R64_S2)
FAMILY = {f: [c for c, r in CODES.items() if r[0] == f] for f in ("reg", "ring32", "ring64", "ring64-half", "p8", "wres", "halo")}
FAMILY["heuristic"] = [0]
B1_CASE = {"reg": "rows40_72_200", "ring32": "rows40_72_200", "ring64": "rows264_328_264", "ring64-half": "c3_12x20_40_40", "p8": "c3_8x32_128_64",
           "wres": "rows300_320_320", "halo": "c3_8x32_128_64", "heuristic": "rowbias24_16_40"}
S1P1 = ("c3_16x8_64_72", "c3_8x32_128_64", "c3_12x20_40_40", "in_16x16_4_64", "out_16x16_64_4")
PASSES = ("primal", "tangent", "adjoint")
_MEASURED = {}                                        # (family, dtype, pass) -> largest |got - ref| / bound of the real tier
_PREP = {}                                            # (case, dtype, tier, B, kps) -> inputs and references, computed once for all the tests


def _dt(dtype):
    return str(dtype).split(".")[-1]


def _case_gathers(case):
    return "n" if case.plain else ("u" if any(s["up"] for s in case.steps) else "c")


def _cases_of(code):
    """the cases a forced code runs: those whose gather its kernel is built for (the halo code: the 3x3 stride-1 pad-1 cases)"""
    if code == 600:
        return [R.CASES[n] for n in S1P1]
    if code == 0:
        return list(R.CASES.values())
    return [c for c in R.CASES.values() if _case_gathers(c) in CODES[code][2]]


def _prepared(case, dtype, tier, B, kps):
    key = (case.name, dtype, tier, B, kps)
    if key not in _PREP:
        g = torch.Generator().manual_seed(zlib.crc32(f"{case.name}|{tier}|{B}".encode()))
        params = R.make_params(case, g, tier, dtype)
        x, V, U = R.make_inputs(case, g, tier, dtype, B, kps)
        ts = (0.0,) * B if tier == "exact" or not case.rowbias else tuple(case.t_real[:B])
        if tier == "exact":
            R.check_exact_precondition(case, params, x, V, U, dtype, kps, ts)
            want = R.exact_reference(case, params, x, V, U, dtype, kps, ts)
            bounds = None
        else:
            want = R.reference(case, params, x, V, U, dtype, kps, ts)
            S = R.magnitude(case, params, x, V, U, dtype, kps, ts)
            slack = R.temb_slack(case, params, dtype, ts, B)
            bounds = tuple(R.real_bound(case, w, r, s, dtype, slack) for w, r, s in zip(PASSES, want, S))
        _PREP[key] = (params, x, V, U, ts, want, bounds)
    return _PREP[key]


def _halo_ok(case, row):
    s = case.steps[-1]
    if len(case.steps) != 1 or s["ks"] != 3 or s["stride"] != 1 or s["pad"] != 1 or s["up"] or row["gather"] not in (1, 2) or (row["K"] // 9) % 64:
        return False
    H, W = case.hw
    hw = H * W
    if row["M"] % hw:
        return False
    if hw >= 256:
        return 256 % W == 0 and hw % 256 == 0 and (256 // W + 2) * (W + 2) <= 400
    return 256 % hw == 0 and W >= 8 and (256 // hw) * (H + 2) * (W + 2) <= 400


def _expected_kind(code, dtype, case, row, which):
    """the profile kind of one product under a forced code: pick_async_tile / pick_reg_tile / wants_halo restated (None: the heuristic decides)"""
    if dtype == F32:
        return 1 if code == 128 else 0                # fp32 never leaves the register-staged kernel
    fam, kind, builds, cin64 = CODES[code]
    if fam == "reg":
        return kind
    if fam == "halo":
        return 5 if _halo_ok(case, row) else None
    takes = "nccu"[row["gather"]] in builds and not (cin64 and row["gather"] and (row["K"] // 9) % 64)
    if fam == "wres":                                 # K = 320, N % 320 == 0, from 32 rows on, at most one row operand: no bias, no row bias
        operand = which == "primal" and any(s["bias"] or s["rowbias"] for s in case.steps)
        takes = takes and row["K"] == 320 and row["N"] % 320 == 0 and row["M"] >= 32 and not operand
    return kind if takes else SUBSTITUTE_KIND


def _expected_split(dtype, row, forced=3):
    """the clamp of gemm_plan on a forced split count: one K step per split at least -- 64-channel chunks (halo kernel), the register-staged kernel's
    chunk (4 x 4 fp32, 4 x 8 16-bit elements), 32 (rings); the weights-resident kernel has no split path"""
    if row["big"] == 12:
        return 1
    if row["big"] == 5:
        return min(forced, (row["K"] // 9) // 64)
    kstep = 16 if dtype == F32 else 32
    return min(forced, (row["K"] + kstep - 1) // kstep)


def _profile_rows(e, x, V, U, ts, path):
    """one primal + jvp + vjp with profiling on -> the product brackets of each pass"""
    e.profile(True)
    R.run_engine(e, x, V, U, ts)
    e.profile_dump(str(path))
    e.profile(False)
    with open(path) as fh:
        rows = [{k: int(r[k]) for k in ("big", "gather", "M", "N", "K")} for r in csv.DictReader(fh)]
    return rows


def _split_rows(case, rows):
    n = len(case.steps)
    per = {"primal": n + (1 if case.rowbias else 0), "tangent": n, "adjoint": n}
    assert len(rows) == sum(per.values()), (case.name, rows)
    out, at = {}, 0
    for w in PASSES:
        out[w] = rows[at:at + per[w]]
        at += per[w]
    return out


def _check(case, dtype, tier, prep, outs, e, what, family):
    params, x, V, U, ts, want, bounds = prep
    for i, w in enumerate(PASSES):
        if tier == "exact":
            R.compare_exact(outs[i], want[i], f"{what} {w}")
        else:
            R.compare_real(outs[i], want[i], bounds[i], f"{what} {w}", _MEASURED, (family, _dt(dtype), w))
    co = case.steps[-1]["cout"]
    if co % 8:                                        # the padding channels of the primal output stay zero
        pad = R.read_padded(e, R.r8(co))[:, co:]
        assert not pad.any(), f"{what}: padded output channels hold {pad.abs().max().item()}"


def _run(family, dtype, tmp_path):
    from diffusion_pullback_amd import lib as L
    lib = L.load()
    dev = torch.device("cuda:0")
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    todo = {}
    for code in FAMILY[family]:
        for case in _cases_of(code):
            todo.setdefault((case.name, 2, 2), []).append(code)
        todo.setdefault((B1_CASE[family], 1, 1), []).append(code)
    t0 = time.time()
    try:
        for (name, B, kps), ccodes in todo.items():
            case = R.CASES[name]
            for tier in ("exact", "real"):
                prep = _prepared(case, dtype, tier, B, kps)
                params, x, V, U, ts = prep[:5]
                e = R.engine(case, R.build_tape(case, params, dtype, dev), B, B * kps)
                x, V, U = x.to(dev), V.to(dev), U.to(dev)
                for code in ccodes:
                    L.check(lib.dpb_debug_set(b"gemm_tile", code))
                    halo = code in (0, 600) and name in S1P1 and dtype != F32
                    counts = {}
                    for split in (0, 1, 3):
                        L.check(lib.dpb_debug_set(b"gemm_splitk", split))
                        for loop in ((1, 0) if halo else (1,)):       # the halo cases on both main loops of the halo kernel
                            L.check(lib.dpb_debug_set(b"halo_loop", loop))
                            what = f"{name} B={B} {dtype} {tier} code {code} splitk {split}" + (f" halo_loop {loop}" if halo else "")
                            outs, n = R.run_engine(e, x, V, U, ts)
                            _check(case, dtype, tier, prep, outs, e, what, family)
                        L.check(lib.dpb_debug_set(b"halo_loop", 1))
                        counts[split] = n
                    if tier != "exact":
                        continue
                    # ---- route proof: the brackets name the forced tile's kind or its substitute's; the forced split ran the reduce kernel
                    L.check(lib.dpb_debug_set(b"gemm_splitk", 0))
                    rows = _split_rows(case, _profile_rows(e, x, V, U, ts, tmp_path / "p.csv"))
                    if code == 600:
                        L.check(lib.dpb_debug_set(b"gemm_tile", 0))
                        rows0 = _split_rows(case, _profile_rows(e, x, V, U, ts, tmp_path / "p.csv"))
                    for pi, w in enumerate(PASSES):
                        for j, row in enumerate(rows[w]):
                            if code == 0:
                                ok = row["big"] in ((0, 1) if dtype == F32 else (0, 1, 2, 3, 4, 5, 6, 11, 12))
                                exp = "a product kind"
                            else:
                                exp = _expected_kind(code, dtype, case, row, w)
                                if exp is None:
                                    exp = rows0[w][j]["big"]
                                ok = row["big"] == exp
                            assert ok, f"{name} B={B} {dtype} code {code} {w} product {j} {row}: bracketed as kind {row['big']}, expected {exp}"
                        more = sum(1 for row in rows[w] if _expected_split(dtype, row) > 1)
                        assert counts[3][pi] - counts[1][pi] == more, (f"{name} B={B} {dtype} code {code} {w}: {counts[3][pi]} launches at splitk 3, "
                                                                       f"{counts[1][pi]} at 1; {more} products stay split: {rows[w]}")
                del e
    finally:
        L.check(lib.dpb_debug_set(b"gemm_tile", 0)); L.check(lib.dpb_debug_set(b"gemm_splitk", 0)); L.check(lib.dpb_debug_set(b"halo_loop", 1))
    torch.cuda.synchronize()
    mx = {k[2]: f"{v:.3f}" for k, v in sorted(_MEASURED.items()) if k[0] == family and k[1] == _dt(dtype)}
    print(f"\nproduct ops: family {family} {dtype}: {sum(len(c) for c in todo.values())} (case, code) pairs in {time.time() - t0:.1f} s; "
          f"real-tier maxima as fractions of the bound: {mx}")


@pytest.mark.parametrize("dtype", [F32, BF, F16], ids=_dt)
def test_register_staged_tiles_match_the_fp64_reference(dtype, tmp_path):
    _run("reg", dtype, tmp_path)


@pytest.mark.parametrize("dtype", [BF, F16], ids=_dt)
def test_bk32_ring_tiles_match_the_fp64_reference(dtype, tmp_path):
    _run("ring32", dtype, tmp_path)


@pytest.mark.parametrize("dtype", [BF, F16], ids=_dt)
def test_bk64_ring_tiles_match_the_fp64_reference(dtype, tmp_path):
    _run("ring64", dtype, tmp_path)


@pytest.mark.parametrize("dtype", [BF, F16], ids=_dt)
def test_bk64_half_tiles_match_the_fp64_reference(dtype, tmp_path):
    _run("ring64-half", dtype, tmp_path)


@pytest.mark.parametrize("dtype", [BF, F16], ids=_dt)
def test_eight_phase_tile_matches_the_fp64_reference(dtype, tmp_path):
    _run("p8", dtype, tmp_path)


@pytest.mark.parametrize("dtype", [BF, F16], ids=_dt)
def test_weights_resident_kernel_matches_the_fp64_reference(dtype, tmp_path):
    _run("wres", dtype, tmp_path)


@pytest.mark.parametrize("dtype", [BF, F16], ids=_dt)
def test_halo_tile_convolution_matches_the_fp64_reference(dtype, tmp_path):
    _run("halo", dtype, tmp_path)


@pytest.mark.parametrize("dtype", [F32, BF, F16], ids=_dt)
def test_heuristic_dispatch_matches_the_fp64_reference(dtype, tmp_path):
    _run("heuristic", dtype, tmp_path)
