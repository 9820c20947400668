"""CPU-only checks of what tests/test_gpu_epilogue_ops.py stands on: the fp64 reference (tests/_norm_ref.py) of the nets of tests/_epilogue_ref.py
and the restated rules by which a product takes a fused epilogue, against the library's own host-only dispatch (dpb_debug_gemm_plan)."""
import ctypes as C

import pytest
import torch

import _epilogue_ref as E
import _norm_ref as R

BF, F16, F32 = R.BF, R.F16, R.F32


def _inputs(seed, B, kps, rows, cin, cout, scale):
    g = torch.Generator().manual_seed(seed)
    x = scale * torch.randn(B, rows, cin, generator=g, dtype=torch.float64)
    V = torch.randn(B * kps, rows, cin, generator=g, dtype=torch.float64)
    U = torch.randn(B * kps, rows, cout, generator=g, dtype=torch.float64)
    return g, x, V, U


@pytest.mark.parametrize("kind", ["G3", "G2"])
@pytest.mark.parametrize("F", [64, 192])
def test_interleaved_net_is_the_split_net_in_fp64(kind, F):
    """the 64-interleave permutes the columns of h and GEGLU undoes it: primal, tangent and adjoint of the il = 64 net are those of the il = 0 net
    (every output element is the same sum of the same products; the bound allows the matrix product another blocking of its fp64 sums)"""
    C_, rows, B, kps = 24, 5, 2, 2
    g, x, V, U = _inputs(F, B, kps, rows, C_, C_ if kind == "G3" else F, 3.0)
    params = E.geglu_params(g, F, C_)
    a = R.reference(E.geglu_net(kind, F, C_, 64), params, x, F32, V, U, kps)
    b = R.reference(E.geglu_net(kind, F, C_, 0), params, x, F32, V, U, kps)
    for p, u, v in zip(E.PASSES, a, b):
        assert u.dtype == torch.float64 and float((u - v).abs().max()) <= 1e-13 * float(v.abs().max()), (kind, F, p, float((u - v).abs().max()))
    # ... and the restated layout is the tape's: a0 g0 a1 g1 ... (one block: F = 64 is the split layout itself)
    h64 = R.evaluate(E.geglu_net(kind, F, C_, 64)[:1], params, x, F32)
    h0 = R.evaluate(E.geglu_net(kind, F, C_, 0)[:1], params, x, F32)
    assert torch.equal(h64, h0) == (F == 64) and torch.equal(h64, h0[..., R.interleave_perm(F, 64)])
    assert torch.equal(h64[..., 64:128], h0[..., F:F + 64])          # the second 64-column block of the interleaved layout is g-block 0


@pytest.mark.parametrize("net", ["G3", "L2"])
def test_reference_derivatives_match_central_differences(net):
    """tangent: (f(x + e V) - f(x - e V)) / 2e; adjoint: <U, J V> = <J^T U, V> with the tangent just checked.  fp64, e = 1e-6: truncation e^2 |f'''|
    ~ 1e-12, rounding 2^-53 |f| / e ~ 1e-10 relative"""
    B, kps, rows = 2, 2, 5
    if net == "G3":
        F, C_ = 64, 24
        g, x, V, U = _inputs(1, B, kps, rows, C_, C_, 3.0)
        steps, params = E.geglu_net("G3", F, C_, 64), E.geglu_params(g, F, C_)
    else:
        K, co = 24, 16
        g, x, V, U = _inputs(2, B, kps, rows, K, co, 1.0)
        steps, params = E.ln_net("L2", co), E.ln_params(g, K, co)
    _, dO, gX = R.reference(steps, params, x, F32, V, U, kps)
    idx = torch.arange(B * kps) // kps
    eps = 1e-6
    f = lambda xx: R.evaluate(steps, params, xx, F32)
    fd = (f(x[idx] + eps * V) - f(x[idx] - eps * V)) / (2 * eps)
    assert float((fd - dO).norm() / dO.norm()) < 1e-8, float((fd - dO).norm() / dO.norm())
    lhs, rhs = (U * dO).sum(dim=(1, 2)), (gX * V).sum(dim=(1, 2))
    assert float((lhs - rhs).abs().max() / lhs.abs().max()) < 1e-12, (lhs, rhs)


# the (rows, B, kps, C) of the GPU file: the main shape, the edge shapes, the heuristic pair
SHAPES = [(77, 2, 2, 72), (7, 2, 2, 72), (77, 1, 1, 72), (77, 1, 3, 72), (77, 2, 2, 64), (77, 1, 2, 2048), (77, 1, 2, 72)]


def test_restated_fuse_rule_is_the_dispatch():
    """dpb_debug_gemm_plan refuses a product with epilogue 1 / 2 / 5 (GEGLU tangent / adjoint / forward) exactly where the restated rule says the
    engine does not fuse; where it plans one, the tile is the one the rule names.  The forward epilogue also needs the plain product unsplit:
    the plan's split count of the plain product is the restated one."""
    from diffusion_pullback_amd import lib as L
    lib = L.load()
    DT = {BF: L.DPB_BF16, F16: L.DPB_F16, F32: L.DPB_F32}
    k, t, s = C.c_int(), C.c_int(), C.c_int()

    def plan(dtype, M, N, K, epi):
        rc = lib.dpb_debug_gemm_plan(DT[dtype], M, N, K, 0, 0, epi, 64 << 20, C.byref(k), C.byref(t), C.byref(s))
        return rc, t.value, s.value

    plan_code = {129: 128, 131: 130, 133: 132, 257: 256, 65: 64}          # forced code -> plan code of the BK = 32 ring rows (kGemmTiles)
    n = {True: 0, False: 0}
    try:
        for code in E.ALL_CODES:
            L.check(lib.dpb_debug_set(b"gemm_tile", code))
            for rows, B, kps, C_ in SHAPES:
                for F in (64, 128, 192, 256):
                    for dtype in (BF, F16, F32):
                        for epi, M, N in ((1, B * kps * rows, 2 * F), (2, B * kps * rows, F), (5, B * rows, 2 * F)):
                            want = E.geglu_fuses(dtype, code, M, N, C_)
                            rc, tile, split = plan(dtype, M, N, C_, epi)
                            assert (rc == 0) == want, (code, rows, B, kps, C_, F, dtype, epi, rc, want)
                            n[want] += 1
                            if want:
                                row = E.epilogue_tile(code, M, N, C_)
                                assert tile == plan_code.get(row, row) and split == 1, (code, epi, M, N, C_, tile, split)
                                rc, tile, split = plan(dtype, M, N, C_, 0)                # the same product, plain: does it split by itself?
                                assert rc == 0 and split == E.plain_split(dtype, code, M, N, C_), (code, M, N, C_, dtype, tile, split)
    finally:
        L.check(lib.dpb_debug_set(b"gemm_tile", 0))
    assert n[True] > 500 and n[False] > 500, n                              # both answers are exercised
    # what the grid is there for, spelled out
    assert not E.geglu_fuses(BF, 65, 308, 256, 72) and not E.geglu_fuses(F32, 515, 308, 256, 72)       # 64-column tile; fp32
    assert E.geglu_fuses(BF, 518, 308, 256, 72) and not E.geglu_fuses(BF, 518, 308, 384, 72)          # 256-column tiles: N % 256
    assert E.geglu_fuses(BF, 515, 308, 384, 72) and not E.geglu_fuses(BF, 515, 308, 192, 72) and not E.geglu_fuses(BF, 515, 308, 64, 72)
    assert E.epilogue_tile(521, 308, 256, 72) == 515 and E.geglu_fuses(BF, 521, 308, 256, 72)         # the half tile hands the product to 515
    assert E.geglu_fuses(BF, 0, 154, 256, 2048) and not E.geglu_fuses(BF, 0, 154, 256, 72)            # the heuristic: BK = 64 ring from K = 2048
    assert not E.geglu_fwd_fuses(BF, 0, 77, 256, 2048) and E.geglu_fwd_fuses(BF, 515, 154, 256, 72)   # forward: the plain product splits 4-fold


def test_restated_layernorm_rule():
    """the row-complete tile is chosen by the epilogue, not by a code: gemm_epi_supported asks for a 16-bit engine, M >= 128, K % 64 == 0 (and
    operands dpb_debug_gemm_plan cannot state, so the GPU file proves this rule by launch counts); conv_adj adds K <= 1024 unless ln_fuse & 2"""
    ex = E.ln_expected
    assert ex(BF, 1, 64, 64, 77, 2, 2) == {"primal": 0, "tangent": 1, "adjoint": 1}
    assert ex(BF, 0, 64, 64, 77, 2, 2) == {"primal": 0, "tangent": 0, "adjoint": 0} == ex(F32, 1, 64, 64, 77, 2, 2)
    assert ex(F16, 1, 72, 64, 77, 1, 2) == {"primal": 0, "tangent": 0, "adjoint": 1}
    assert ex(F16, 1, 320, 64, 77, 1, 1) == {"primal": 0, "tangent": 0, "adjoint": 0}                  # M = 77 < 128
    assert ex(BF, 1, 128, 1280, 77, 2, 2)["adjoint"] == 0 and ex(BF, 3, 128, 1280, 77, 2, 2)["adjoint"] == 1
