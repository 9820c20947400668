"""CPU-only: the dispatch of the folded text-attention epilogue (EPI_XATT = 6, csrc/epilogue.h) -- one of the two BK = 64 ring tiles that are built
with it, never split over K, whatever the heuristic would give the same shape with a plain epilogue."""
import ctypes as C

import pytest

from diffusion_pullback_amd import lib as L


def _plan(M, N, K, epi, dtype=L.DPB_BF16):
    l = L.load()
    kind, tile, split = C.c_int(), C.c_int(), C.c_int()
    r = l.dpb_debug_gemm_plan(dtype, M, N, K, 0, 0, epi, 64 << 20, C.byref(kind), C.byref(tile), C.byref(split))
    return r, tile.value, split.value


@pytest.mark.parametrize("M,K,tile", [(64, 640, 521), (320, 1280, 521), (1280, 1280, 521), (5120, 640, 515), (20480, 320, 515)])
def test_xatt_products_take_a_128_column_ring_tile_unsplit(M, K, tile):
    """N = 128 columns per head, 8 heads: the 64 x 128 half tile while 128 x 128 tiles would number fewer than 256, the 128 x 128 ring from there on"""
    for dtype in (L.DPB_BF16, L.DPB_F16):
        assert _plan(M, 1024, K, 6, dtype) == (0, tile, 1)


def test_xatt_is_refused_where_no_kernel_has_it():
    assert _plan(320, 1024, 1280, 6, L.DPB_F32)[0] != 0          # 16-bit engines only
    assert _plan(320, 1000, 1280, 6)[0] != 0                     # whole 128-column head windows only
