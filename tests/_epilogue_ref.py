"""The fused product epilogues (csrc/epilogue.h: EPI_GEGLU_TAN / _ADJ / _FWD, EPI_LN_TAN / _ADJ) at op level: the nets that reach them, their
parameters, and the rules by which the dispatch decides that a launch fuses, restated.  The fp64 reference and the comparator are tests/_norm_ref.py;
tests/test_epilogue_ops_host.py checks the restated rules against dpb_debug_gemm_plan without a GPU.

The 64-interleave of the FF-in weight rows (Tape.conv(..., interleave=64)) only permutes the columns of h, and GEGLU with il = 64 undoes it: the
reference of an interleaved net is the reference of the same net with il = 0 (asserted in fp64 by the host file), and that net on the engine -- the
`il = 0` arm -- can never fuse: its kernels are the plain products and the stand-alone GEGLU kernel, pinned by test_gpu_product_ops.py and
test_gpu_norm_ops.py.
"""
import math

import torch

import _norm_ref as R

BF, F16, F32 = R.BF, R.F16, R.F32
PASSES = ("primal", "tangent", "adjoint")
LN_WIDTH = 320                                         # the row-complete tile (code 520): N = 320 exactly

# forced code -> (tile columns bn, built with the GEGLU epilogues (TILE_GEGLU), fused epilogues need N % 256 == 0 (TILE_EPI_N256), profile kind as
# include/dpb.h documents it, never splits K by itself (TILE_NOSPLIT), family) -- the rows of kGemmTiles (csrc/kernels.h) this file forces
TILES = {
    129: (128, True, False, 2, False, "ring32"), 131: (128, True, False, 2, False, "ring32"), 133: (128, True, False, 2, False, "ring32"),
    257: (128, True, False, 2, False, "ring32"), 65: (64, True, False, 3, False, "ring32"),
    512: (128, True, False, 4, False, "ring64"), 513: (128, True, False, 4, False, "ring64"), 514: (128, True, False, 4, False, "ring64"),
    515: (128, True, False, 4, False, "ring64"), 516: (128, True, False, 4, False, "ring64"), 517: (128, True, False, 4, False, "ring64"),
    518: (256, True, True, 6, True, "ring64"), 521: (128, False, False, 4, False, "ring64"), 530: (256, True, True, 11, True, "p8"),
}
SUBSTITUTE = 515                                       # the row that runs a product a forced tile is not built for (kGemmTiles: T_R64_S2)
FUSING_CODES = (129, 131, 133, 257, 512, 513, 514, 515, 516, 517, 518, 530)     # TILE_GEGLU and bn % 128 == 0
ALL_CODES = FUSING_CODES + (65, 521, 0)                # + the 64-column ring, the half tile (not built with the epilogues), the heuristic
BODY_CODES = (129, 257, 515, 516, 518, 530)            # one code per distinct kernel body


# =============================================================================================== nets
def geglu_net(kind: str, F: int, C: int, il: int):
    """G3: h = linear(x, 2F), y = geglu(h), o = linear(y, C) -- tangent epilogue in the first product, adjoint epilogue in the adjoint of the second;
    G2: the first two steps, tap on y -- the tangent and forward epilogues alone"""
    steps = [R.linear("h", "x", "ffin", 2 * F, interleave=il), R.geglu("y", "h", il)]
    if kind == "G3":
        steps.append(R.linear("o", "y", "ffout", C))
    return steps


def geglu_params(g: torch.Generator, F: int, C: int):
    return {"ffin.weight": torch.randn(2 * F, C, generator=g) / math.sqrt(C), "ffin.bias": 0.5 * torch.randn(2 * F, generator=g),
            "ffout.weight": torch.randn(C, F, generator=g) / math.sqrt(F), "ffout.bias": 0.5 * torch.randn(C, generator=g)}


def ln_net(kind: str, cout: int):
    """L1: h = linear(x, 320), z = ln(h), o = linear(z, cout);  L2: h = linear(x, 320) + linear(x, 320) (EPI_LN_TAN adds R before it rounds);
    L3: o = concat(linear(z, cout), h): h has a later reader -- the adjoint epilogue accumulates, the tangent's C store is read back"""
    steps = []
    if kind == "L2":
        steps += [R.linear("r", "x", "pr", LN_WIDTH), R.linear("h", "x", "p1", LN_WIDTH, res="r")]
    else:
        steps.append(R.linear("h", "x", "p1", LN_WIDTH))
    steps.append(R.ln("z", "h", "n"))
    if kind == "L3":
        steps += [R.linear("q", "z", "p2", cout), R.concat("o", "q", "h")]
    else:
        steps.append(R.linear("o", "z", "p2", cout))
    return steps


def ln_params(g: torch.Generator, K: int, cout: int):
    p = R.norm_params(g, ["n"], LN_WIDTH)
    for name, co, ci in (("p1", LN_WIDTH, K), ("pr", LN_WIDTH, K), ("p2", cout, LN_WIDTH)):
        p[name + ".weight"] = torch.randn(co, ci, generator=g) / math.sqrt(ci)
        p[name + ".bias"] = 0.5 * torch.randn(co, generator=g)
    return p


# =============================================================================================== the route rules, restated
def _cdiv(a, b):
    return (a + b - 1) // b


def heuristic_tile(M: int, N: int, K: int):
    """pick_async_tile without a forced code, for a product with a fused epilogue at the sizes of these tests (few tiles): the register-staged
    kernel (None) below K = 256; the BK = 64 ring 515 from K = 2048 on.  (The half-tile rules ask for a plain epilogue.)"""
    assert _cdiv(M, 256) * _cdiv(N, 256) < 160 and M < 49152, "a size at which the 8-phase, 256 x 256 or weights-resident tiles compete"
    if K < 256:
        return None
    t128 = _cdiv(M, 128) * _cdiv(N, 128)
    if K >= 512 and (t128 >= 200 or K >= 2048):
        return 515
    raise NotImplementedError((M, N, K))


def epilogue_tile(code: int, M: int, N: int, K: int):
    """the tile row that runs a plain-row product with a GEGLU epilogue under a forced code (pick_async_tile): the forced row if its kernel is built
    with the epilogues, else that row's substitute; code 0: the heuristic.  None: the register-staged kernel."""
    if code == 0:
        return heuristic_tile(M, N, K)
    return code if TILES[code][1] else SUBSTITUTE


def geglu_fuses(dtype, code: int, M: int, N: int, K: int) -> bool:
    """gemm_epi_supported for EPI_GEGLU_TAN / _FWD (N = 2F) and EPI_GEGLU_ADJ (N = F): a 16-bit engine, whole 128-column blocks, the product's tile
    built with the epilogues and made of whole 128-column blocks, and N % 256 == 0 on the 256-column tiles"""
    if dtype == F32 or N % 128:
        return False
    t = epilogue_tile(code, M, N, K)
    if t is None:
        return False
    bn, built, n256 = TILES[t][:3]
    return built and bn % 128 == 0 and (not n256 or N % 256 == 0)


def plain_split(dtype, code: int, M: int, N: int, K: int) -> int:
    """the K split the dispatch gives the PLAIN product by itself (pick_splitk), at the sizes of these tests: the forward epilogue is for products
    that run unsplit anyway"""
    assert dtype != F32
    nk = _cdiv(K, 32)
    if code == 0:
        if K < 256:
            return 1                                   # register-staged 64 x 64 tile: fewer than 32 K chunks
        t128 = _cdiv(M, 128) * _cdiv(N, 128)           # K >= 2048: ring 515 (or its half tile: the same family rule at these tile counts)
        assert K >= 2048 and t128 < 192
        half = M % 128 and M % 128 <= 64               # the 64-row half tile covers M exactly
        tiles = _cdiv(M, 64) * _cdiv(N, 128) if half else t128
        return min(max(1, (448 + tiles // 2) // tiles), max(1, nk // 16))
    bn, _, _, _, nosplit, fam = TILES[code]
    if nosplit:
        return 1
    bm = {129: 128, 131: 128, 133: 128, 257: 256, 65: 64, 512: 128, 513: 256, 514: 128, 515: 128, 516: 256, 517: 256, 521: 64}[code]
    tiles = _cdiv(M, bm) * _cdiv(N, bn)
    if fam == "ring32":
        return 1 if tiles >= 256 or nk < 64 else min(_cdiv(1024, tiles), nk // 12, 32)
    if tiles >= 192:
        return 2 if tiles < 256 and nk >= 128 else 1
    return min(max(1, (448 + tiles // 2) // tiles), max(1, nk // 16))


def geglu_fwd_fuses(dtype, code: int, M: int, N: int, K: int) -> bool:
    """conv_fwd: dpb_forward applies GEGLU in the FF-in product's epilogue when the epilogue is supported and the plain product would run unsplit"""
    return geglu_fuses(dtype, code, M, N, K) and plain_split(dtype, code, M, N, K) == 1


def geglu_expected(kind: str, dtype, code: int, F: int, C: int, rows: int, B: int, kps: int):
    """{pass: number of GEGLU launches the pass saves} for G3 / G2 with il = 64, and the same for dpb_forward"""
    M = B * kps * rows
    tan = geglu_fuses(dtype, code, M, 2 * F, C)
    adj = kind == "G3" and geglu_fuses(dtype, code, M, F, C)
    return {"primal": 0, "tangent": int(tan), "adjoint": int(adj), "forward": int(geglu_fwd_fuses(dtype, code, B * rows, 2 * F, C))}


def ln_expected(dtype, ln_fuse: int, K: int, cout: int, rows: int, B: int, kps: int):
    """{pass: LayerNorm launches saved} under dpb_debug_set("ln_fuse", v): gemm_epi_supported for the row-complete tile (16-bit, at least one 128-row
    tile, K % 64 == 0) and conv_adj's K <= 1024 unless bit 1 of the switch is set.  K of the adjoint product is the width of the product's output."""
    M = B * kps * rows
    ok = ln_fuse != 0 and dtype != F32 and M >= 128
    return {"primal": 0, "tangent": int(ok and K % 64 == 0), "adjoint": int(ok and cout % 64 == 0 and (cout <= 1024 or bool(ln_fuse & 2)))}
