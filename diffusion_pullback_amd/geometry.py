"""Principal angles and geodesic distances between local tangent spaces -- the analysis the bases (u, s, vT) of
``run_sample_encoder_local_tangent_space_zt`` are saved for.

For two k-dimensional subspaces of R^N with principal angles theta_1 >= ... >= theta_k the geodesic distance on the Grassmannian is
``||theta||_2``.  The work is on the GPU (``csrc/angles.hip``): one exact fp64 cross-Gram of all rows on the fp64 matrix cores, then fp64 small
algebra per basis and per pair; see ``include/dpb.h`` for the method, the limits and the NaN rule.  Held to ``scipy.linalg.subspace_angles`` in
float64 at 1e-6 rad per angle -- small angles included, which the usual fp32 ``qr`` / ``svdvals`` / ``arccos`` route misses by 1e-4 .. 7e-4 rad.

Distances only: no exponential / logarithm maps, no Frechet means, no parallel transport.  There is no CPU fallback: inputs live on a HIP device.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import lib as L

MAX_RANK = 128                       # ORTH_MAX_RANK of the library
DEFAULT_MAX_BYTES = 4 << 30          # device scratch of one call (the fp64 cross-Gram of the block dominates: 8 (B k)^2 bytes)


def _device_f32(t, what: str) -> torch.Tensor:
    if not torch.is_tensor(t) or not t.is_cuda:
        raise L.DpbError(f"{what} must be a tensor on a HIP device (there is no CPU fallback)")
    if not t.is_floating_point():
        raise ValueError(f"{what} must have a floating-point dtype, got {t.dtype}")
    return t.detach().to(dtype=torch.float32).contiguous()


def cross_gram(X: torch.Tensor, Y: Optional[torch.Tensor] = None) -> torch.Tensor:
    """G = X Y^T in float64 from fp32 rows: X [Ra, N], Y [Rb, N] (None: Y = X; the tiles above the diagonal are computed and mirrored, G is exactly
    symmetric).  Products are exact, the accumulation is fp64 in a fixed order (dpb_cross_gram): bitwise reproducible, and an entry does not depend on
    Ra, Rb or its position.  No host sync."""
    lib = L.load()
    X = _device_f32(X, "X")
    if X.dim() != 2 or X.numel() == 0:
        raise ValueError(f"X must be a non-empty [Ra, N] matrix, got {tuple(X.shape)}")
    if Y is not None:
        Y = _device_f32(Y, "Y").to(X.device)
        if Y.dim() != 2 or Y.shape[1] != X.shape[1] or Y.shape[0] == 0:
            raise ValueError(f"Y must be [Rb, N = {X.shape[1]}], got {tuple(Y.shape)}")
    ra, n = X.shape
    rb = ra if Y is None else Y.shape[0]
    with torch.cuda.device(X.device):
        st = torch.cuda.current_stream(X.device).cuda_stream
        G = torch.empty(ra, rb, dtype=torch.float64, device=X.device)
        L.check(lib.dpb_cross_gram(X.data_ptr(), None if Y is None else Y.data_ptr(), G.data_ptr(), ra, rb, n, C.c_void_p(st)))
    return G


def _stack(t, what: str) -> torch.Tensor:
    t = _device_f32(t, what)
    if t.dim() == 2:                                   # one basis
        t = t[None]
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError(f"{what} must be a stack of bases [B, k, N] (or one basis [k, N]), got {tuple(t.shape)}")
    return t


def _block(lib, ba: int, bb: int, k: int, n: int, self_mode: bool, max_bytes: int) -> int:
    """bases per block: the largest b whose call -- b x b (self mode), b x min(b, Bb) otherwise -- keeps scratch + Gram within max_bytes (at least 1)"""
    need = lambda b: int(lib.dpb_subspace_angles_scratch_bytes(min(b, ba), min(b, bb), k, n))
    lo, hi = 1, max(ba, bb)
    if need(hi) <= max_bytes:
        return hi
    while lo < hi:                                     # need() grows with b
        mid = (lo + hi + 1) // 2
        if need(mid) <= max_bytes:
            lo = mid
        else:
            hi = mid - 1
    return lo


def subspace_angles_and_distance(A: torch.Tensor, B: Optional[torch.Tensor] = None, max_bytes: Optional[int] = None,
                                 check: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """theta [Ba, Bb, k] (fp32, descending per pair) and dist [Ba, Bb] = ||theta||_2 between every basis of A [Ba, k, N] and every basis of B
    [Bb, k, N] (None: self mode -- A against itself, pairs i < j computed and mirrored, an exactly zero diagonal).  A [k, N] tensor is one basis;
    any float dtype is converted to contiguous fp32.  Rows need not be orthonormal, only independent.  When one call's scratch (its fp64 cross-Gram
    included) would exceed max_bytes the pairs go through in blocks of bases; a pair's result does not depend on the call it is computed in, so the
    result is bitwise the one-call result.  check: raise ValueError naming the degenerate bases (NaN rows / columns; one host sync); False returns
    the NaNs."""
    lib = L.load()
    A = _stack(A, "A")
    self_mode = B is None
    Bs = A if self_mode else _stack(B, "B").to(A.device)
    ba, k, n = A.shape
    bb = Bs.shape[0]
    if tuple(Bs.shape[1:]) != (k, n):
        raise ValueError(f"A holds bases of k = {k} rows of length N = {n}, B of k = {Bs.shape[1]}, N = {Bs.shape[2]}: they must match")
    if k > MAX_RANK:
        raise ValueError(f"k = {k} rows per basis exceeds the supported rank {MAX_RANK}")
    if k > n:
        raise ValueError(f"k = {k} rows per basis exceeds their length N = {n}: they cannot be independent")
    max_bytes = DEFAULT_MAX_BYTES if max_bytes is None else int(max_bytes)
    with torch.cuda.device(A.device):
        st = C.c_void_p(torch.cuda.current_stream(A.device).cuda_stream)
        blk = _block(lib, ba, bb, k, n, self_mode, max_bytes)
        need = int(lib.dpb_subspace_angles_scratch_bytes(min(blk, ba), min(blk, bb), k, n))
        if need == 0:
            raise L.DpbError(f"dpb_subspace_angles does not take Ba = {ba}, Bb = {bb}, k = {k}, N = {n}")
        scratch = torch.empty(need, dtype=torch.uint8, device=A.device)
        theta = torch.empty(ba, bb, k, dtype=torch.float32, device=A.device)
        dist = torch.empty(ba, bb, dtype=torch.float32, device=A.device)

        def call(a, b, na, nb, th, di):
            L.check(lib.dpb_subspace_angles(a.data_ptr(), None if b is None else b.data_ptr(), na, nb, k, n, th.data_ptr(), di.data_ptr(),
                                            scratch.data_ptr(), need, st))
        if blk >= max(ba, bb):
            call(A, None if self_mode else Bs, ba, bb, theta, dist)
        else:
            for i0 in range(0, ba, blk):
                i1 = min(i0 + blk, ba)
                for j0 in range(i0 if self_mode else 0, bb, blk):
                    j1 = min(j0 + blk, bb)
                    th = torch.empty(i1 - i0, j1 - j0, k, dtype=torch.float32, device=A.device)
                    di = torch.empty(i1 - i0, j1 - j0, dtype=torch.float32, device=A.device)
                    if self_mode and i0 == j0:
                        call(A[i0:i1], None, i1 - i0, i1 - i0, th, di)
                    else:
                        call(A[i0:i1], Bs[j0:j1], i1 - i0, j1 - j0, th, di)
                    theta[i0:i1, j0:j1] = th
                    dist[i0:i1, j0:j1] = di
                    if self_mode and i0 != j0:         # the mirror image of an off-diagonal block
                        theta[j0:j1, i0:i1] = th.transpose(0, 1)
                        dist[j0:j1, i0:i1] = di.t()
    if check:
        bad = torch.isnan(dist)
        if bool(bad.any()):
            rows = bad.all(dim=1).nonzero().flatten().tolist()
            cols = bad.all(dim=0).nonzero().flatten().tolist()
            if self_mode:
                raise ValueError(f"degenerate bases (a zero row, or rows dependent beyond a condition number of ~1e5): indices {rows}")
            raise ValueError(f"degenerate bases (a zero row, or rows dependent beyond a condition number of ~1e5): indices {rows} of A, {cols} of B")
    return theta, dist


def subspace_angles(A: torch.Tensor, B: Optional[torch.Tensor] = None, max_bytes: Optional[int] = None) -> torch.Tensor:
    """Principal angles theta [Ba, Bb, k] in radians, descending per pair (the convention of scipy.linalg.subspace_angles), between the row spans of
    the bases of A [Ba, k, N] and B [Bb, k, N] (None: A against itself).  See subspace_angles_and_distance."""
    return subspace_angles_and_distance(A, B, max_bytes)[0]


def geodesic_distance(A: torch.Tensor, B: Optional[torch.Tensor] = None, max_bytes: Optional[int] = None) -> torch.Tensor:
    """Geodesic distance on the Grassmannian, dist [Ba, Bb] = ||theta||_2 over the principal angles of each pair.  See subspace_angles_and_distance."""
    return subspace_angles_and_distance(A, B, max_bytes)[1]
