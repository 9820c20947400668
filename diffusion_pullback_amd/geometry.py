"""Principal angles and geodesic distances between local tangent spaces -- the analysis the bases (u, s, vT) of
``run_sample_encoder_local_tangent_space_zt`` are saved for.

For two k-dimensional subspaces of R^N with principal angles theta_1 >= ... >= theta_k the geodesic distance on the Grassmannian is
``||theta||_2``.  The work is on the GPU (``csrc/angles.hip``): one exact fp64 cross-Gram of all rows on the fp64 matrix cores, then fp64 small
algebra per basis and per pair; see ``include/dpb.h`` for the method, the limits and the NaN rule.  Held to ``scipy.linalg.subspace_angles`` in
float64 at 1e-6 rad per angle -- small angles included, which the usual fp32 ``qr`` / ``svdvals`` / ``arccos`` route misses by 1e-4 .. 7e-4 rad.

``transport_directions`` is the direction arithmetic of ``run_edit_parallel_transport`` (``csrc/transport.hip``): a source direction of h-space
expressed in a target's basis and carried to the target's x-space, fp64 on the h-space side, a fixed-order fp32 stream on the x-space side.

``flag_mean`` is the flag (extrinsic, chordal) mean of many such bases -- the global basis of ``run_edit_global_flag_mean_zt`` (``csrc/flagmean.hip``):
the top eigenvectors of the mean projector, by block subspace iteration on the same whitened fp64 Gram; closed form, any rank, nested, and its
spectrum says how many directions the local spaces share.

``flag_mean(weights=)`` and ``flag_median`` are the weighted flag mean and the flag median (FlagIRLS) of the same bases -- the L1 counterpart, on which
outlying members pull with a bounded force and whose final weights rank the members from typical to outlying: the same solver on the Gram scaled
inside its one pass, a round per reweighting, warm-started.

``flag_affinity`` is the chordal affinity sum_j cos^2 theta_j = ||Q_Y Q_A^T||_F^2 between subspaces of different rank, and ``flag_kmeans`` clusters many
bases into several families, each with a flag mean as its centre -- Lloyd's algorithm on that affinity (``csrc/flagkmeans.hip``), the analysis of
``run_tangent_space_clusters``: on the same whitened Gram, the flag-mean solver per cluster, one pass over the Gram per round for all clusters.

``frechet_mean`` is the Frechet (Karcher) mean on the Grassmannian of many such bases -- the global basis of ``run_edit_global_frechet_mean_zt``
(``csrc/frechet.hip``): the Riemannian fixed-step iteration on coefficients against the whitened fp64 Gram of all rows, one streaming pass over the
rows before it and one after it.

``linear_assignment`` and ``hungarian_mean`` are the other global basis, of ``run_edit_global_hungarian_mean_zt`` (``csrc/hungarian.hip``): the
directions of every basis matched one to one and sign by sign to an anchor's by a batched assignment solver on the device, and the matched unit
vectors averaged in one streaming pass -- a mean of directions, where the Frechet mean is a mean of subspaces.

``principal_vectors``, ``grassmann_log``, ``grassmann_geodesic`` and ``grassmann_exp`` are the geodesics of the Grassmannian between pairs of such
bases (``csrc/geodesic.hip``): which directions two tangent spaces share, the tangent that leads from one to the other, the points of the geodesic
between them (interpolated or extrapolated) and the geodesic shot from a space along a tangent -- per pair from the exact fp64 Grams, then one
streaming pass that holds both rotated tiles in registers and writes every output slice from them.

``grassmann_pga`` is principal geodesic analysis of many such bases around a centre (``csrc/pga.hip``), the analysis of ``run_tangent_space_pga``: PCA of
the log maps at the Frechet mean (or the flag mean, a member, any base) -- the modes that carry the spread, every member's scores on them, and the
tangent-space regression on covariates such as the timestep -- from the Gram of the tangents, which closes in k x k algebra on the whitened Gram the
mean has formed, then one streaming synthesis of the modes.

There is no CPU fallback: inputs live on a HIP device.
"""
from __future__ import annotations

import ctypes as C
import time
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as L

MAX_RANK = 128                       # ORTH_MAX_RANK of the library
FRECHET_MAX_RANK = 64                # FRECHET_MAX_RANK of the library (three k x k fp64 matrices of the log map live in LDS)
DEFAULT_MAX_BYTES = 4 << 30          # device scratch of one call (the fp64 cross-Gram of the block dominates: 8 (B k)^2 bytes)

DEGENERATE = "degenerate bases (a zero row, or rows dependent beyond a condition number of ~1e5)"


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
                raise ValueError(f"{DEGENERATE}: indices {rows}")
            raise ValueError(f"{DEGENERATE}: indices {rows} of A, {cols} of B")
    return theta, dist


def transport_directions(u_src: torch.Tensor, u_dst: torch.Tensor, vT_dst: torch.Tensor, pcs: Optional[Sequence[int]] = None,
                         check: bool = True) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The directions of run_edit_parallel_transport (dpb_transport_directions): the source's h-space direction u_src[pc], expressed in each
    target's h-space basis and carried to x-space through that target's own u / vT pairing.

    Layout: ROWS.  u_src [k, N_h]; u_dst [D, k, N_h] with vT_dst [D, k, N_x], or one target as u_dst [k, N_h] with vT_dst [k, N_x].  The saved files
    hold ``u-`` as [N_h, k] columns and ``vT-`` as [k, N_x] rows: pass ``u.t()`` (any strides; inputs are made contiguous fp32).  Rows need not be
    normalised.  pcs: the components of the source to transport, entries in [0, k) in any order (None: all k).

    Returns vk [D, P, N_x] (unit norm), coef [D, P, k] with coef[d, p] = Uhat_d^T uhat_src[pcs[p]], and coef_norm [D, P] = ||coef[d, p]||_2: the share
    of the source direction that the target's h-tangent space holds (its cosine to that space only when Uhat_d is orthonormal).  The result of a
    target is bitwise the same alone and inside any stack.  check: raise ValueError naming the degenerate (target, pc) pairs -- a zero or non-finite
    source row, a zero target row, a target exactly orthogonal to the direction; one host sync -- False returns their NaNs.  No CPU fallback."""
    lib = L.load()
    u_src = _device_f32(u_src, "u_src")
    if u_src.dim() != 2 or u_src.numel() == 0:
        raise ValueError(f"u_src must be one basis [k, N_h] of rows, got {tuple(u_src.shape)}")
    u_dst = _stack(u_dst, "u_dst").to(u_src.device)
    vT_dst = _stack(vT_dst, "vT_dst").to(u_src.device)
    k, nh = u_src.shape
    d, nx = vT_dst.shape[0], vT_dst.shape[2]
    if tuple(u_dst.shape) != (d, k, nh) or vT_dst.shape[1] != k:
        raise ValueError(f"u_src is [k = {k}, N_h = {nh}]: u_dst must be [D, {k}, {nh}] and vT_dst [D, {k}, N_x] with the same D, got "
                         f"{tuple(u_dst.shape)} and {tuple(vT_dst.shape)}")
    if k > MAX_RANK:
        raise ValueError(f"k = {k} rows per basis exceeds the supported rank {MAX_RANK}")
    pcs = list(range(k)) if pcs is None else [int(p) for p in pcs]
    if not 1 <= len(pcs) <= k or any(p < 0 or p >= k for p in pcs):
        raise ValueError(f"pcs must hold 1 .. k = {k} entries in [0, {k}), got {pcs}")
    npc = len(pcs)
    with torch.cuda.device(u_src.device):
        st = C.c_void_p(torch.cuda.current_stream(u_src.device).cuda_stream)
        need = int(lib.dpb_transport_scratch_bytes(d, npc, k, nh, nx))
        if need == 0:
            raise L.DpbError(f"dpb_transport_directions does not take D = {d}, P = {npc}, k = {k}, N_h = {nh}, N_x = {nx}")
        scratch = torch.empty(need, dtype=torch.uint8, device=u_src.device)
        vk = torch.empty(d, npc, nx, dtype=torch.float32, device=u_src.device)
        coef = torch.empty(d, npc, k, dtype=torch.float32, device=u_src.device)
        coef_norm = torch.empty(d, npc, dtype=torch.float32, device=u_src.device)
        L.check(lib.dpb_transport_directions(u_src.data_ptr(), u_dst.data_ptr(), vT_dst.data_ptr(), (C.c_int32 * npc)(*pcs), npc, d, k, nh, nx,
                                             vk.data_ptr(), coef.data_ptr(), coef_norm.data_ptr(), scratch.data_ptr(), need, st))
    if check:
        bad = torch.isnan(coef_norm) | torch.isnan(vk).any(dim=2)
        if bool(bad.any()):
            pairs = [(int(i), pcs[int(j)]) for i, j in bad.nonzero().tolist()]
            raise ValueError("degenerate transport (a zero or non-finite source row, a zero target row, or a target exactly orthogonal to the "
                             f"direction): (target, pc) pairs {pairs}")
    return vk, coef, coef_norm


FLAG_MEAN_MAX_RANK = 64              # FLAG_MEAN_MAX_RANK of the library (the block of the subspace iteration is at most 64 columns wide)


def _flag_solve(lib, b: int, k: int, n: int, r: int, max_iter: int, tol: float, check_every: int, seed: int, X, ghat, scratch, need: int, st):
    """init and the chunked iteration of dpb_flag_mean_* on X (ghat None) or on a caller's Ghat; the status read after a chunk is the only sync"""
    L.check(lib.dpb_flag_mean_init(None if X is None else X.data_ptr(), ghat, b, k, n, r, seed, max_iter, scratch.data_ptr(), need, st))
    asked = 0
    while asked < max_iter:
        steps = min(check_every, max_iter - asked)
        L.check(lib.dpb_flag_mean_iterate(steps, float(tol), ghat, b, k, n, r, max_iter, scratch.data_ptr(), need, st))
        asked += steps
        if int(scratch[:4].view(torch.int32).item()) != 0:
            break


def _flag_info(raw: np.ndarray, b: int, r: int, weight, theta) -> dict:
    m = int(raw[3])
    eig = raw[8:8 + m] / b
    return {"iterations": int(raw[0]), "converged": int(raw[1]) == 1, "residual": float(raw[2]), "weight": weight, "eigenvalues": eig.copy(),
            "gap": float(eig[r - 1] - eig[r]) if m > r else None, "theta": theta, "degenerate": np.nonzero(raw[72:72 + b] != 0)[0].tolist()}


def _member_weights(weights, b: int, device) -> torch.Tensor:
    """the caller's member weights as a [B] fp64 device tensor; ValueError naming the offending indices (the one host check, and its sync)"""
    w = weights.detach().to("cpu", torch.float64).numpy() if torch.is_tensor(weights) else np.asarray(weights, dtype=np.float64)
    if w.shape != (b,):
        raise ValueError(f"weights must hold one value per basis, [B = {b}], got shape {tuple(w.shape)}")
    bad = np.nonzero(~np.isfinite(w) | (w < 0))[0].tolist()
    if bad:
        raise ValueError(f"weights must be finite and >= 0: indices {bad}")
    if not w.sum() > 0:
        raise ValueError(f"weights must have a positive sum: all {b} are zero")
    return torch.from_numpy(np.ascontiguousarray(w)).to(device)


def _median_head(scratch: torch.Tensor) -> dict:
    """the head of a dpb_flag_median_* block (include/dpb.h): one device read"""
    raw = scratch[:64].cpu().numpy()
    i, d = raw[:24].view(np.int32), raw[24:48].view(np.float64)
    return {"round": int(i[0]), "done": int(i[1]), "iters": int(i[2]), "n_degenerate": int(i[3]), "converged": int(i[4]) != 0, "J": float(d[0]),
            "J_prev": float(d[1]), "res": float(d[2])}


def _median_run(lib, A: torch.Tensor, r: int, w_dev, do_rounds: bool, max_rounds: int, eps: float, tol: float, inner_iter: int, inner_tol: float,
                check_every: int, seed: int, max_bytes: int, what: str):
    """dpb_flag_median_*: init, then per round the chunked inner solve and (do_rounds) the round step, then finish.  do_rounds False is the weighted mean"""
    b, k, n = A.shape
    need = int(lib.dpb_flag_median_scratch_bytes(b, k, n, r, inner_iter))
    if need == 0:
        raise L.DpbError(f"dpb_flag_median does not take B = {b}, k = {k}, N = {n}, r = {r}, max_iter = {inner_iter}")
    if need > max_bytes:
        raise ValueError(f"{what} of B = {b} bases of k = {k} rows needs {need} bytes of device scratch (the fp64 Gram of all {b * k} rows), "
                         f"max_bytes is {max_bytes}")
    d = min(r, k)
    objective, inner_its, inner_conv, converged = [], [], [], False
    with torch.cuda.device(A.device):
        st = C.c_void_p(torch.cuda.current_stream(A.device).cuda_stream)
        dev = A.device
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        Y = torch.empty(r, n, dtype=torch.float32, device=dev)
        weight = torch.empty(r, dtype=torch.float32, device=dev)
        theta = torch.empty(b, d, dtype=torch.float32, device=dev)
        Ct = torch.empty(b * k, r, dtype=torch.float64, device=dev)
        member = torch.empty(3, b, dtype=torch.float64, device=dev)
        info_d = torch.empty(72 + b, dtype=torch.float64, device=dev)
        sp = scratch.data_ptr()
        L.check(lib.dpb_flag_median_init(A.data_ptr(), None, None if w_dev is None else w_dev.data_ptr(), b, k, n, r, seed, inner_iter, sp, need, st))
        while True:
            asked = 0
            while asked < inner_iter:
                steps = min(check_every, inner_iter - asked)
                L.check(lib.dpb_flag_median_iterate(steps, float(inner_tol), None, b, k, n, r, inner_iter, sp, need, st))
                asked += steps
                if _median_head(scratch)["done"] != 0:                 # the one host read of the chunk
                    break
            if not do_rounds:
                break
            update = len(objective) < max_rounds
            L.check(lib.dpb_flag_median_round(float(eps), float(tol), 1 if update else 0, None, b, k, n, r, inner_iter, sp, need, st))
            head = _median_head(scratch)                                # the one host read of the round
            objective.append(head["J"])
            inner_its.append(head["iters"])
            inner_conv.append(head["done"] == 1)
            converged = head["converged"]
            if converged or not update or head["done"] == 2 or head["J"] != head["J"]:
                break
        L.check(lib.dpb_flag_median_finish(A.data_ptr(), None, Y.data_ptr(), weight.data_ptr(), theta.data_ptr(), Ct.data_ptr(), member.data_ptr(),
                                           info_d.data_ptr(), b, k, n, r, inner_iter, sp, need, st))
        raw = info_d.cpu().numpy()
    info = _flag_info(raw, b, r, weight, theta)
    info.update({"affinity": member[0], "distance": member[1], "member_weight": member[2]})
    return Y, info, objective, inner_its, inner_conv, converged


def flag_mean(A: torch.Tensor, rank: Optional[int] = None, max_iter: int = 1000, tol: float = 1e-12, check_every: int = 16, seed: int = 0,
              max_bytes: Optional[int] = None, check: bool = True, weights=None) -> Tuple[torch.Tensor, dict]:
    """The flag (extrinsic, chordal) mean of the row spans of A [B, k, N]: the top ``rank`` eigenvectors of the mean projector (1/B) sum_i Q_i^T Q_i
    over the orthonormalised members (Draper et al. 2014) -- closed form, no cut locus, defined for every rank in [1, min(64, B k, N)] (None: k), and
    nested: rows 0 .. j-1 are the rank-j mean (dpb_flag_mean_init / _iterate / _finish; see include/dpb.h for the method and the limits).  Rows need
    not be orthonormal, only independent; any float dtype is converted to contiguous fp32; k <= 64.

    Returns Y [rank, N] fp32 with orthonormal rows in descending eigenvalue order and info: ``iterations``, ``converged`` (the relative residual of
    the top ``rank`` Ritz pairs fell to tol), ``residual`` (the last one computed), ``weight`` [rank] (fp32: eigenvalue j, the mean cos^2 with which the
    members hold row j), ``eigenvalues`` (fp64 numpy: all m Ritz values of the solver's block, the oversampled ones included -- a gap in them is the
    number of directions the members share), ``gap`` (weight[rank-1] minus the next one; None when the block is no wider than rank), ``theta``
    [B, min(rank, k)] (fp32: the principal angles of span Y to every member, descending) and ``degenerate``.

    Block subspace iteration with a Rayleigh-Ritz step per iteration on the whitened fp64 Gram of all B k rows, in chunks of check_every iterations
    with one status read per chunk.  Not converging within max_iter is not an error -- it is the answer when row ``rank`` sits inside the bulk of the
    spectrum: converged is False, Y is still orthonormal and weight its Rayleigh quotients.  The Gram must fit max_bytes (8 (B k)^2 bytes plus the
    block).  check: raise ValueError naming the degenerate bases; False returns the NaNs.  Bitwise reproducible for a given seed (the start block).

    weights (None: the call above, untouched): a length-B tensor or sequence, finite, >= 0, with a positive sum -- the weighted flag mean, the top
    eigenvectors of sum_i w_i Q_i^T Q_i / sum_i w_i (dpb_flag_median_* with no round: the same solver, the weights applied inside the pass over the Gram).
    A member of weight 0 is excluded from the mean and still gets its row of ``theta``; ``weight`` and ``eigenvalues`` are those of the weighted
    projector; info gains ``member_weight`` [B] (the weights scaled to mean 1) and ``affinity`` [B] (sum_j cos^2 of each member to span Y), fp64 on
    the device.  Bad weights raise ValueError naming the indices (one host check).  Uniform weights return the unweighted call's bits."""
    lib = L.load()
    A = _stack(A, "A")
    b, k, n = A.shape
    if k > FRECHET_MAX_RANK:
        raise ValueError(f"k = {k} rows per basis exceeds the rank {FRECHET_MAX_RANK} the flag mean supports")
    if k > n:
        raise ValueError(f"k = {k} rows per basis exceeds their length N = {n}: they cannot be independent")
    r = k if rank is None else int(rank)
    top = min(FLAG_MEAN_MAX_RANK, b * k, n)
    if not 1 <= r <= top:
        raise ValueError(f"rank = {r} outside [1, min({FLAG_MEAN_MAX_RANK}, B k = {b * k}, N = {n}) = {top}]")
    max_iter, check_every, seed = int(max_iter), int(check_every), int(seed)
    if max_iter < 0 or check_every < 1 or not tol >= 0 or seed < 0:
        raise ValueError(f"max_iter = {max_iter} must be >= 0, check_every = {check_every} >= 1, tol = {tol} >= 0 and seed = {seed} >= 0")
    max_bytes = DEFAULT_MAX_BYTES if max_bytes is None else int(max_bytes)
    if weights is not None:
        w_dev = _member_weights(weights, b, A.device)
        Y, info, _, _, _, _ = _median_run(lib, A, r, w_dev, False, 0, 1.0, 0.0, max_iter, tol, check_every, seed, max_bytes, "the weighted flag mean")
        info.pop("distance")
        if check and info["degenerate"]:
            raise ValueError(f"{DEGENERATE}: indices {info['degenerate']}")
        return Y, info
    need = int(lib.dpb_flag_mean_scratch_bytes(b, k, n, r, max_iter))
    if need == 0:
        raise L.DpbError(f"dpb_flag_mean does not take B = {b}, k = {k}, N = {n}, r = {r}, max_iter = {max_iter}")
    if need > max_bytes:
        raise ValueError(f"the flag mean of B = {b} bases of k = {k} rows needs {need} bytes of device scratch (the fp64 Gram of all {b * k} rows), "
                         f"max_bytes is {max_bytes}")
    d = min(r, k)
    with torch.cuda.device(A.device):
        st = C.c_void_p(torch.cuda.current_stream(A.device).cuda_stream)
        scratch = torch.empty(need, dtype=torch.uint8, device=A.device)
        Y = torch.empty(r, n, dtype=torch.float32, device=A.device)
        weight = torch.empty(r, dtype=torch.float32, device=A.device)
        theta = torch.empty(b, d, dtype=torch.float32, device=A.device)
        Ct = torch.empty(b * k, r, dtype=torch.float64, device=A.device)
        info_d = torch.empty(72 + b, dtype=torch.float64, device=A.device)
        _flag_solve(lib, b, k, n, r, max_iter, tol, check_every, seed, A, None, scratch, need, st)
        L.check(lib.dpb_flag_mean_finish(A.data_ptr(), None, Y.data_ptr(), weight.data_ptr(), theta.data_ptr(), Ct.data_ptr(), info_d.data_ptr(),
                                         b, k, n, r, max_iter, scratch.data_ptr(), need, st))
        raw = info_d.cpu().numpy()
    info = _flag_info(raw, b, r, weight, theta)
    if check and info["degenerate"]:
        raise ValueError(f"{DEGENERATE}: indices {info['degenerate']}")
    return Y, info


def flag_median(A: torch.Tensor, rank: Optional[int] = None, eps: float = 1e-5, max_rounds: int = 50, tol: float = 1e-9, inner_iter: int = 200,
                inner_tol: float = 1e-12, check_every: int = 16, seed: int = 0, weights=None, max_bytes: Optional[int] = None,
                check: bool = True) -> Tuple[torch.Tensor, dict]:
    """The flag median of the row spans of A [B, k, N] (Mankovich, King, Peterson, Kirby, CVPR 2022, FlagIRLS): the rank-``rank`` subspace (None: k;
    1 <= rank <= k) minimising sum_i p_i d_i with d_i = sqrt(rank - a_i) the chordal distance -- not its square, which the flag mean minimises -- and
    a_i = ||Q_i Y^T||_F^2, so that outlying members pull with a bounded force.  Iteratively reweighted flag means (dpb_flag_median_*; include/dpb.h):
    round 0 is the flag mean under the prior weights p (``weights``; None: uniform), every further round the weighted flag mean under
    w_i = p_i / max(d_i, eps), scaled to mean 1; the inner solve of a round (at most inner_iter iterations to inner_tol in chunks of check_every) is
    warm-started at the previous round's block.  The objective is J = sum_i p_i phi(d_i), phi(d) = d for d >= eps and d^2 / (2 eps) + eps / 2 below
    it: what IRLS with the clamped weight descends.  The run stops when J_prev - J <= tol J_prev (``converged``) or after max_rounds reweightings;
    max_rounds = 0 is the (weighted) flag mean and its objective.

    eps = 1e-5: the affinity's recorded worst error is 5.7e-12 (k = rank = 64), so sqrt(rank - a) has a floor near 2.4e-6; eps sits above that floor,
    and a member lying in span Y gets a large, finite weight.

    Returns Y [rank, N] fp32 (orthonormal rows, descending Rayleigh quotient) and info: ``rounds`` (reweightings taken), ``converged``, ``objective``
    (fp64 numpy, one entry per round, the start included), ``monotone`` (no entry rose by more than 1e-12 J), ``member_weight`` [B] (the weights of
    the last solve, mean 1: low for outlying members), ``distance`` [B] and ``affinity`` [B] (to the returned Y; fp64 on the device), ``weight``
    [rank] (fp32: the Rayleigh quotients of the weighted mean projector of the last round), ``eigenvalues``, ``gap``, ``theta`` [B, rank] (as
    flag_mean's), ``inner_iterations`` (per round), ``inner_converged`` (all of them) and ``degenerate``.  Not converging, an inner solve that does
    not settle (row ``rank`` inside the bulk of the spectrum) and monotone = False are reported, not raised.  check: raise ValueError naming the
    degenerate bases; False returns the NaNs.  One host read per round and one per chunk of the inner solves.  Bitwise reproducible."""
    lib = L.load()
    A = _stack(A, "A")
    b, k, n = A.shape
    if k > FRECHET_MAX_RANK:
        raise ValueError(f"k = {k} rows per basis exceeds the rank {FRECHET_MAX_RANK} the flag median supports")
    if k > n:
        raise ValueError(f"k = {k} rows per basis exceeds their length N = {n}: they cannot be independent")
    r = k if rank is None else int(rank)
    if not 1 <= r <= k:
        raise ValueError(f"rank = {r} outside [1, k = {k}]: the chordal distance sqrt(rank - a) is defined for rank <= k only")
    max_rounds, inner_iter, check_every, seed = int(max_rounds), int(inner_iter), int(check_every), int(seed)
    if not eps > 0 or max_rounds < 0 or inner_iter < 0 or check_every < 1 or not tol >= 0 or not inner_tol >= 0 or seed < 0:
        raise ValueError(f"eps = {eps} must be > 0, max_rounds = {max_rounds} and inner_iter = {inner_iter} >= 0, check_every = {check_every} >= 1, "
                         f"tol = {tol} and inner_tol = {inner_tol} >= 0 and seed = {seed} >= 0")
    max_bytes = DEFAULT_MAX_BYTES if max_bytes is None else int(max_bytes)
    w_dev = None if weights is None else _member_weights(weights, b, A.device)
    Y, info, objective, inner_its, inner_conv, converged = _median_run(lib, A, r, w_dev, True, max_rounds, eps, tol, inner_iter, inner_tol, check_every,
                                                                       seed, max_bytes, "the flag median")
    objective = np.asarray(objective, dtype=np.float64)
    info.pop("iterations"); info.pop("residual")
    info.update({"rounds": len(objective) - 1, "converged": bool(converged), "objective": objective,
                 "monotone": bool(np.all(objective[1:] <= objective[:-1] * (1.0 + 1e-12))), "inner_iterations": inner_its,
                 "inner_converged": bool(all(inner_conv))})
    if check and info["degenerate"]:
        raise ValueError(f"{DEGENERATE}: indices {info['degenerate']}")
    return Y, info


def frechet_mean(A: torch.Tensor, init=0, max_iter: int = 1000, tol: float = 1e-6, step: float = 1.0, check_every: int = 16,
                 max_bytes: Optional[int] = None, check: bool = True) -> Tuple[torch.Tensor, dict]:
    """The Frechet (Karcher) mean on the Grassmannian of the row spans of A [B, k, N]: the k-dimensional subspace Y minimising
    (1 / 2B) sum_i ||theta(Y, A_i)||_2^2, by Y <- Exp_Y(step * mean_i Log_Y(A_i)) started at the span of A[init] (dpb_frechet_init / _iterate / _finish;
    see include/dpb.h for the method and the limits).  Rows need not be orthonormal, only independent; any float dtype is converted to contiguous fp32.

    Returns Y [k, N] fp32 with orthonormal rows in canonical order -- row 0 is the direction the members share most -- and info: ``iterations``
    (steps taken), ``converged`` (the gradient norm ||mean Log||_F fell below tol), ``grad_norm`` (the last one computed), ``cost`` (fp64 numpy history
    of (1/2) mean_i sum theta^2, the start included, iterations + 1 entries), ``grad_norm_history``, ``weight`` [k] (fp32, descending: the mean cos^2
    with which the members hold each row of Y) and ``theta`` [B, k] (fp32: the principal angles of Y to every member, descending).

    The iteration runs in chunks of check_every steps with no host sync inside a chunk; the status read after each chunk is the only sync, and the steps
    of a chunk after convergence are empty launches.  Not reaching tol within max_iter is not an error: converged is False.  The fp64 Gram of all B k
    rows must fit max_bytes (8 (B k)^2 bytes plus the coefficient buffers).  check: raise ValueError naming the degenerate bases, or the basis whose
    largest principal angle to the iterate left the log map's domain (pi/2 - 1e-6); False returns the NaNs and, in info, ``degenerate`` and ``domain``.
    A cost that rises by more than 1e-12 relative between two steps raises DpbError: the step is too long for this set.  Bitwise reproducible.

    init="flag" starts at the rank-k flag mean instead of a member (flag_mean: central, so no member is near pi/2 from it): the flag solver runs on the
    whitened Gram this call has already formed -- there is no second pass over the rows -- for at most 64 iterations (to a residual of 1e-10), and
    dpb_frechet_start takes its coefficients; info then holds ``flag_iterations`` and ``flag_converged``.  Any other string raises ValueError."""
    A = _stack(A, "A")
    Y, info, _ = _frechet_run(A, init, max_iter, tol, step, check_every, max_bytes, check, 0)
    return Y, info


def _frechet_run(A: torch.Tensor, init, max_iter: int, tol: float, step: float, check_every: int, max_bytes: Optional[int], check: bool, extra_bytes: int):
    """frechet_mean on a stacked fp32 A, its Frechet scratch block kept: (Y, info, (scratch, need, max_iter)).  extra_bytes: device memory the caller will
    allocate next to it (counted against max_bytes)"""
    lib = L.load()
    b, k, n = A.shape
    if k > FRECHET_MAX_RANK:
        raise ValueError(f"k = {k} rows per basis exceeds the rank {FRECHET_MAX_RANK} the Frechet mean supports")
    if k > n:
        raise ValueError(f"k = {k} rows per basis exceeds their length N = {n}: they cannot be independent")
    from_flag = isinstance(init, str)
    if from_flag and init != "flag":
        raise ValueError(f"init must be the index of a member or 'flag', got {init!r}")
    init, max_iter, check_every = 0 if from_flag else int(init), int(max_iter), int(check_every)
    if not 0 <= init < b:
        raise ValueError(f"init = {init} outside [0, B = {b})")
    if max_iter < 0 or check_every < 1 or not tol >= 0 or not step > 0:
        raise ValueError(f"max_iter = {max_iter} must be >= 0, check_every = {check_every} >= 1, tol = {tol} >= 0 and step = {step} > 0")
    max_bytes = DEFAULT_MAX_BYTES if max_bytes is None else int(max_bytes)
    need = int(lib.dpb_frechet_scratch_bytes(b, k, n, max_iter))
    if need == 0:
        raise L.DpbError(f"dpb_frechet does not take B = {b}, k = {k}, N = {n}, max_iter = {max_iter}")
    if need + extra_bytes > max_bytes:
        raise ValueError(f"the Frechet mean of B = {b} bases of k = {k} rows needs {need + extra_bytes} bytes of device scratch (the fp64 Gram of all {b * k} rows), "
                         f"max_bytes is {max_bytes}")
    with torch.cuda.device(A.device):
        st = C.c_void_p(torch.cuda.current_stream(A.device).cuda_stream)
        scratch = torch.empty(need, dtype=torch.uint8, device=A.device)
        Y = torch.empty(k, n, dtype=torch.float32, device=A.device)
        weight = torch.empty(k, dtype=torch.float32, device=A.device)
        theta = torch.empty(b, k, dtype=torch.float32, device=A.device)
        info_d = torch.empty(8 + 2 * max_iter + 1 + b, dtype=torch.float64, device=A.device)
        L.check(lib.dpb_frechet_init(A.data_ptr(), b, k, n, init, max_iter, scratch.data_ptr(), need, st))
        flag_raw = None
        if from_flag:
            flag_iter = 64                                   # (a start, not an answer: row k may sit inside the bulk, where the block never settles)
            fneed = int(lib.dpb_flag_mean_solver_bytes(b, k, k, flag_iter))
            ghat = lib.dpb_frechet_ghat(b, k, n, max_iter, scratch.data_ptr())
            if fneed == 0 or not ghat:
                raise L.DpbError(f"dpb_flag_mean does not take B = {b}, k = {k}, r = {k} on the Frechet mean's Gram")
            if need + extra_bytes + fneed > max_bytes:
                raise ValueError(f"the flag start of the Frechet mean needs {fneed} more bytes of device scratch, max_bytes is {max_bytes}")
            fscratch = torch.empty(fneed, dtype=torch.uint8, device=A.device)
            fCt = torch.empty(b * k, k, dtype=torch.float64, device=A.device)
            finfo = torch.empty(72 + b, dtype=torch.float64, device=A.device)
            _flag_solve(lib, b, k, n, k, flag_iter, 1e-10, check_every, 0, None, ghat, fscratch, fneed, st)
            L.check(lib.dpb_flag_mean_finish(None, ghat, None, weight.data_ptr(), theta.data_ptr(), fCt.data_ptr(), finfo.data_ptr(), b, k, n, k,
                                             flag_iter, fscratch.data_ptr(), fneed, st))
            L.check(lib.dpb_frechet_start(fCt.data_ptr(), b, k, n, max_iter, scratch.data_ptr(), need, st))
            flag_raw = finfo.cpu().numpy()
        asked = 0
        while asked < max_iter:
            steps = min(check_every, max_iter - asked)
            L.check(lib.dpb_frechet_iterate(steps, float(step), float(tol), b, k, n, max_iter, scratch.data_ptr(), need, st))
            asked += steps
            if int(scratch[:4].view(torch.int32).item()) != 0:          # status.done: the one host sync of the chunk
                break
        L.check(lib.dpb_frechet_finish(A.data_ptr(), Y.data_ptr(), weight.data_ptr(), theta.data_ptr(), info_d.data_ptr(), b, k, n, max_iter,
                                       scratch.data_ptr(), need, st))
        raw = info_d.cpu().numpy()
    iters, done, domain = int(raw[0]), int(raw[2]), int(raw[3])
    cost = raw[8:8 + iters + 1].copy()
    ghist = raw[8 + max_iter + 1:8 + max_iter + 1 + iters + (1 if done == 1 else 0)].copy()
    degenerate = np.nonzero(raw[8 + 2 * max_iter + 1:] != 0)[0].tolist()
    info = {"iterations": iters, "converged": done == 1, "grad_norm": float(ghist[-1]) if len(ghist) else float("nan"), "cost": cost,
            "grad_norm_history": ghist, "weight": weight, "theta": theta, "degenerate": degenerate, "domain": domain if done == 2 else None}
    if flag_raw is not None:
        info["flag_iterations"], info["flag_converged"] = int(flag_raw[0]), int(flag_raw[1]) == 1
    if check:
        if degenerate:
            raise ValueError(f"{DEGENERATE}: indices {degenerate}")
        if done == 2:
            raise ValueError(f"basis {domain} left the log map's domain at step {iters}: its largest principal angle to the iterate exceeds pi/2 - 1e-6 "
                             f"(start from another init, or drop the basis)")
    if raw[5] != 0 and not degenerate:
        raise L.DpbError("frechet_mean: the iterate lost rank (its Gram has a pivot below 1e-10): use a smaller step")
    rise = cost[1:] - cost[:-1]
    worst = np.nonzero(rise > 1e-12 * cost[:-1] + 1e-15 * k)[0]        # (1e-15 k: the rounding floor of k squared angles from fp64 sin^2)
    if len(worst):
        j = int(worst[0])
        raise L.DpbError(f"frechet_mean: the cost rose from {cost[j]!r} to {cost[j + 1]!r} at step {j + 1}: use a smaller step than {step}")
    return Y, info, (scratch, need, max_iter)


CUT_LOCUS = "pairs at the cut locus (largest principal angle above pi/2 - 1e-6: the geodesic is not unique there)"


def _times(ts) -> list:
    ts = [float(ts)] if isinstance(ts, (int, float)) else [float(t) for t in ts]
    if not 1 <= len(ts) <= 64:
        raise ValueError(f"ts must hold 1 .. 64 parameters, got {len(ts)}")
    return ts


def _grassmann_call(X, Y, mode: int, ts, check: bool, max_bytes: Optional[int], names: Tuple[str, str]):
    """the one driver of the four public calls: mode 0 principal vectors, 1 log, 2 geodesic (dpb_grassmann_pair), 3 exp (dpb_grassmann_exp)"""
    lib = L.load()
    X, Y = _device_f32(X, names[0]), _device_f32(Y, names[1])       # (both on a device before any shape is judged: no CPU fallback)
    broadcast = mode != 3 and X.dim() == 2 and Y.dim() == 3
    X = _stack(X, names[0])
    Y = _stack(Y, names[1]).to(X.device)
    d, k, n = Y.shape
    if tuple(X.shape[1:]) != (k, n) or (X.shape[0] != d and not broadcast):
        raise ValueError(f"{names[1]} holds {d} bases of k = {k} rows of length N = {n}: {names[0]} must be [{d}, {k}, {n}]"
                         + ("" if mode == 3 else f" or one basis [{k}, {n}]") + f", got {tuple(X.shape)}")
    if k > FRECHET_MAX_RANK:
        raise ValueError(f"k = {k} rows per basis exceeds the rank {FRECHET_MAX_RANK} the Grassmann geodesics support")
    if k > n:
        raise ValueError(f"k = {k} rows per basis exceeds their length N = {n}: they cannot be independent")
    timed = mode >= 2
    ts = _times(ts) if timed else []
    j = len(ts) if timed else 2
    max_bytes = DEFAULT_MAX_BYTES if max_bytes is None else int(max_bytes)
    need = int(lib.dpb_grassmann_scratch_bytes(d, j, k, n))
    if need == 0:
        raise L.DpbError(f"dpb_grassmann does not take D = {d}, J = {j}, k = {k}, N = {n}")
    if need > max_bytes:
        raise ValueError(f"the Grassmann geodesics of D = {d} pairs of k = {k} rows need {need} bytes of device scratch, max_bytes is {max_bytes}")
    with torch.cuda.device(X.device):
        st = C.c_void_p(torch.cuda.current_stream(X.device).cuda_stream)
        scratch = torch.empty(need, dtype=torch.uint8, device=X.device)
        spec = torch.empty(d, k, dtype=torch.float32, device=X.device)
        flags = torch.empty(d, dtype=torch.int32, device=X.device)
        tarr = (C.c_double * max(len(ts), 1))(*ts)
        if timed:
            out0 = torch.empty(d, j, k, n, dtype=torch.float32, device=X.device)
            out1 = None
        else:
            out0 = torch.empty(d, k, n, dtype=torch.float32, device=X.device)
            out1 = torch.empty(d, k, n, dtype=torch.float32, device=X.device)
        if mode == 3:
            L.check(lib.dpb_grassmann_exp(X.data_ptr(), Y.data_ptr(), d, k, n, tarr, j, out0.data_ptr(), spec.data_ptr(), flags.data_ptr(),
                                          scratch.data_ptr(), need, st))
        else:
            L.check(lib.dpb_grassmann_pair(X.data_ptr(), 0 if broadcast else k * n, Y.data_ptr(), d, k, n, mode, tarr, j, out0.data_ptr(),
                                           None if out1 is None else out1.data_ptr(), spec.data_ptr(), flags.data_ptr(), scratch.data_ptr(), need, st))
    if check:
        fl = flags.cpu().numpy()                                    # the one host sync
        if (fl == 1).any():
            raise ValueError(f"{DEGENERATE}: indices {np.nonzero(fl == 1)[0].tolist()}")
        if (fl == 2).any():
            raise ValueError(f"{CUT_LOCUS}: indices {np.nonzero(fl == 2)[0].tolist()}")
    return out0, out1, spec


def principal_vectors(A: torch.Tensor, B: torch.Tensor, check: bool = True, max_bytes: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The principal vectors of the pairs (A[d], B[d]): Pa [D, k, N] in span A[d] and Pb [D, k, N] in span B[d], both with orthonormal rows, and
    theta [D, k] (fp32, descending: the order of subspace_angles) with Pa[d] Pb[d]^T = diag(cos theta[d]), cos theta >= 0 -- row i of the two is the
    pair of directions the spaces hold at angle theta_i (dpb_grassmann_pair, mode 0; see include/dpb.h for the method, the sign rule and the limits).

    Layout: ROWS.  A and B [D, k, N]; A [k, N] against a stack B [D, k, N] is broadcast; [k, N] with [k, N] is D = 1 (the leading axis is kept).  Rows
    need not be orthonormal, only independent; any float dtype is converted to contiguous fp32; k <= 64.  A pair's result is bitwise the same alone,
    at any position of a stack and broadcast.  check: raise ValueError naming the degenerate pairs, or the pairs at the cut locus (largest angle
    above pi/2 - 1e-6); one host sync -- False returns their NaNs.  No CPU fallback."""
    pa, pb, theta = _grassmann_call(A, B, 0, None, check, max_bytes, ("A", "B"))
    return pa, pb, theta


def grassmann_log(A: torch.Tensor, B: torch.Tensor, check: bool = True, max_bytes: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The log map at span A[d] of span B[d] as (P, H, theta): P [D, k, N] an orthonormal basis of span A[d] (the principal vectors on A's side) and H
    [D, k, N] the images of its rows -- the tangent is the linear map p_i -> h_i = (theta_i / sin theta_i)(pb_i - cos theta_i p_i).  h_i is orthogonal
    to span A[d], ||h_i|| = theta_i, and ||H[d]||_F is the geodesic distance.  grassmann_exp(P, H, t) walks the geodesic: t = 1 arrives at span B[d].
    Pairing, inputs, check and limits as principal_vectors (dpb_grassmann_pair, mode 1)."""
    p, h, theta = _grassmann_call(A, B, 1, None, check, max_bytes, ("A", "B"))
    return p, h, theta


def grassmann_geodesic(A: torch.Tensor, B: torch.Tensor, ts, check: bool = True, max_bytes: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Points of the geodesic from span A[d] (t = 0) to span B[d] (t = 1): Y [D, T, k, N] with orthonormal rows, Y[d, j] a basis of the point at
    ts[j], and theta [D, k].  ts: a float or a sequence of up to 64; any real t (beyond [0, 1] the geodesic is extrapolated).  Row i of Y[d, j] is
    sin((1 - t) theta_i) / sin theta_i pa_i + sin(t theta_i) / sin theta_i pb_i over the principal vectors; all T slices are written from one pass
    over the 2k rows.  Pairing, inputs, check and limits as principal_vectors (dpb_grassmann_pair, mode 2)."""
    y, _, theta = _grassmann_call(A, B, 2, ts, check, max_bytes, ("A", "B"))
    return y, theta


def grassmann_exp(P: torch.Tensor, H: torch.Tensor, ts, check: bool = True, max_bytes: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The exp map: the geodesic shot from span P[d] along the tangent (P[d], H[d]), at ts: Y [D, T, k, N] with orthonormal rows and sigma [D, k]
    (fp32, descending: the singular values of the tangent, ||sigma||_2 the speed).  P [D, k, N] any independent rows, H [D, k, N] anything: the tangent
    is the linear map p_i -> the component of h_i orthogonal to span P[d].  With (P, H) of grassmann_log(A, B), Y at t reproduces
    grassmann_geodesic(A, B, t) as a subspace.  No domain limit.  check: raise ValueError naming the pairs whose P is degenerate; one host sync --
    False returns their NaNs (dpb_grassmann_exp; see include/dpb.h).  No CPU fallback."""
    y, _, sigma = _grassmann_call(P, H, 3, ts, check, max_bytes, ("P", "H"))
    return y, sigma


PGA_MAX_MODES = 64                   # the block of the subspace iteration is at most 64 columns wide
PGA_MAX_COVARIATES = 8
PGA_ROUTES = {1: "jacobi", 2: "subspace"}


def _pga_covariates(covariates, b: int) -> np.ndarray:
    x = covariates.detach().to("cpu", torch.float64).numpy() if torch.is_tensor(covariates) else np.asarray(covariates, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    if x.ndim != 2 or x.shape[0] != b or not 1 <= x.shape[1] <= PGA_MAX_COVARIATES:
        raise ValueError(f"covariates must be [B = {b}] or [B = {b}, P <= {PGA_MAX_COVARIATES}], got shape {tuple(np.shape(covariates))}")
    if not np.isfinite(x).all():
        raise ValueError(f"covariates must be finite: members {np.nonzero(~np.isfinite(x).all(axis=1))[0].tolist()}")
    return x


def grassmann_pga(A: torch.Tensor, base="frechet", n_modes: Optional[int] = None, center: bool = True, covariates=None,
                  max_bytes: Optional[int] = None, check: bool = True, **mean_kwargs) -> Tuple[torch.Tensor, torch.Tensor, dict]:
    """Principal geodesic analysis (tangent PCA) of the row spans of A [B, k, N] around a base point: how the members vary around a centre.  With
    L_i = Log_Y(span A_i) -- a [k, N] tangent in the convention of grassmann_log / grassmann_exp: row j is the image of row j of the returned Y and
    L_i Y^T = 0 -- the analysis is ordinary PCA of the B vectors L_i under <L_a, L_b> = tr(L_a L_b^T), centred by their mean when ``center``
    (dpb_pga_tangent_gram / _eig / _combine on the scratch block of the mean; see include/dpb.h for the method, the limits and the NaN rule).

    base: "frechet" -- the Karcher mean; mean_kwargs are frechet_mean's init, max_iter, tol, step, check_every and Y is bitwise what
    frechet_mean(A, ...) returns; "flag" -- the rank-k flag mean, as frechet_mean(init="flag") starts, with no Karcher step; an int -- that member; a
    tensor [k, N] -- any independent rows, in the members' span or not (stacked as one more basis for the Gram, part of no statistic).

    Returns (Y [k, N], modes [M, k, N], info).  Y: orthonormal rows in the canonical order of frechet_mean.  modes (fp32): mode m has unit Frobenius norm,
    modes[m] Y^T = 0, descending variance; its sign makes its largest-magnitude score positive (magnitudes within 1e-9 relative tie; the lowest member wins).  A mode is a tangent at Y:
    grassmann_exp(Y, t * modes[m], 1.0) walks along it.  n_modes (None: min(B - 1, 16) centred, min(B, 16) otherwise) in [1, min(64, B - 1 or B)].

    info: ``variance`` [M] (fp64 numpy: the eigenvalues of the tangent covariance (1/B) sum_i vec(L_i - Lbar) vec(L_i - Lbar)^T, descending),
    ``total_variance`` ((1/B) sum ||L_i - Lbar||^2), ``explained`` [M] (cumulative share; zeros when the total is 0), ``scores`` [B, M] (fp64 on the
    device: <L_i - Lbar, modes[m]>), ``residual`` [B] (fp64: ||L_i - Lbar - sum_m scores[i, m] modes[m]||_F), ``mean_tangent_norm`` (||Lbar||_F: the
    Karcher gradient norm when base="frechet"), ``mean_tangent`` [k, N] (fp32: Lbar itself, so that grassmann_exp(Y, mean_tangent + sum_m scores[i, m]
    modes[m], 1.0) rebuilds member i up to its residual), ``theta`` [B, k] (fp32: principal angles of Y to every member, descending), ``tangent_gram`` [B, B]
    (fp64 on the device, uncentred), ``degenerate`` and ``domain`` (member indices: degenerate, and beyond pi/2 - 1e-6 from the base), ``solver``
    ("jacobi": one workgroup, B <= 128; "subspace": block subspace iteration with a Rayleigh-Ritz step, with ``subspace_iterations`` and
    ``subspace_converged``), and the mean's own ``iterations`` and ``converged`` when a mean was computed.  An eigenvalue not above 1e-13 of the
    largest, or below the rounding floor B k 2^-46 of the Gram, carries no mode: that mode, its variance and its scores are zero (B copies of one basis give zeros, not NaN).

    covariates: [B] or [B, P] (tensor or sequence, P <= 8, finite) asks for the tangent-space least-squares fit L_i ~ L_0 + sum_p x_ip S_p; info gains
    ``slopes`` [P, k, N] and ``intercept`` [k, N] (fp32 tangents at Y), ``r2`` (the share of the centred total variance the fit explains) and
    ``slope_norm`` [P].  The basis predicted at covariate x is grassmann_exp(Y, intercept + sum_p x_p slopes[p], 1.0).  The coefficients of the slopes on
    the L_i depend on the covariates alone and their norms on tangent_gram: the small solve runs on the host in float64.  A rank-deficient centred
    design raises ValueError.

    check: raise ValueError naming the degenerate members, or the members whose largest angle to the base exceeds pi/2 - 1e-6 (the cut locus of the
    log map); False returns NaN in exactly those members' rows and columns of tangent_gram and rows of scores and residual, and forms every statistic
    over the others (a degenerate member still makes Y and the modes NaN: that is frechet_mean's finish).  The fp64 Gram of all rows must fit
    max_bytes.  One host read for the state and the spectrum, one for the covariate fit, plus the mean's own.  Bitwise reproducible.  No CPU fallback."""
    lib = L.load()
    A = _stack(A, "A")
    b, k, n = A.shape
    if k > FRECHET_MAX_RANK:
        raise ValueError(f"k = {k} rows per basis exceeds the rank {FRECHET_MAX_RANK} the Frechet mean supports")
    if k > n:
        raise ValueError(f"k = {k} rows per basis exceeds their length N = {n}: they cannot be independent")
    center = bool(center)
    if center and b < 2:
        raise ValueError(f"B = {b}: a centred analysis needs at least 2 members")
    top = min(PGA_MAX_MODES, b - 1 if center else b)
    m = min(top, 16) if n_modes is None else int(n_modes)
    if not 1 <= m <= top:
        raise ValueError(f"n_modes = {m} outside [1, min({PGA_MAX_MODES}, {'B - 1' if center else 'B'}) = {top}]")
    x = None if covariates is None else _pga_covariates(covariates, b)
    npar = 0 if x is None else x.shape[1]
    rows = m + 1 + (npar + 1 if npar else 0)                  # the modes, the mean tangent, the slopes and the intercept
    stacked, mean_args = A, None
    if isinstance(base, str):
        if base == "frechet":
            bad = sorted(set(mean_kwargs) - {"init", "max_iter", "tol", "step", "check_every"})
            if bad:
                raise TypeError(f"grassmann_pga: unknown arguments {bad} (frechet_mean takes init, max_iter, tol, step, check_every)")
            kw = {"init": 0, "max_iter": 1000, "tol": 1e-6, "step": 1.0, "check_every": 16, **mean_kwargs}
            mean_args = (kw["init"], kw["max_iter"], kw["tol"], kw["step"], kw["check_every"])
        elif base == "flag":
            mean_args = ("flag", 0, 1e-6, 1.0, 16)
        else:
            raise ValueError(f"base must be 'frechet', 'flag', the index of a member or a [k, N] tensor, got {base!r}")
    elif torch.is_tensor(base):
        y0 = _device_f32(base, "base").to(A.device)
        if tuple(y0.shape) != (k, n):
            raise ValueError(f"base must be [k = {k}, N = {n}], got {tuple(y0.shape)}")
        stacked = torch.cat([A, y0[None]])
        mean_args = (b, 0, 1e-6, 1.0, 16)
    else:
        if not 0 <= int(base) < b:
            raise ValueError(f"base = {base} outside [0, B = {b})")
        mean_args = (int(base), 0, 1e-6, 1.0, 16)
    if mean_kwargs and not (isinstance(base, str) and base == "frechet"):
        raise TypeError(f"grassmann_pga: {sorted(mean_kwargs)} belong to base='frechet'")
    bs = stacked.shape[0]
    max_bytes = DEFAULT_MAX_BYTES if max_bytes is None else int(max_bytes)
    pneed = int(lib.dpb_pga_scratch_bytes(bs, b, k, n, rows))
    if pneed == 0:
        raise L.DpbError(f"dpb_pga does not take B = {bs}, members = {b}, k = {k}, N = {n}, J = {rows}")
    Y, minfo, (fscratch, fneed, cap) = _frechet_run(stacked, *mean_args, max_bytes, check, pneed)
    dev = A.device
    with torch.cuda.device(dev):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        scratch = torch.empty(pneed, dtype=torch.uint8, device=dev)
        T = torch.empty(b, b, dtype=torch.float64, device=dev)
        theta = torch.empty(b, k, dtype=torch.float32, device=dev)
        state = torch.empty(b, dtype=torch.int32, device=dev)
        Wt = torch.zeros(rows, b, dtype=torch.float64, device=dev)
        out = torch.empty(72 + b * m + b, dtype=torch.float64, device=dev)
        tangents = torch.empty(rows, k, n, dtype=torch.float32, device=dev)
        L.check(lib.dpb_pga_tangent_gram(bs, b, k, n, cap, rows, fscratch.data_ptr(), fneed, T.data_ptr(), theta.data_ptr(), state.data_ptr(),
                                         scratch.data_ptr(), pneed, st))
        L.check(lib.dpb_pga_eig(T.data_ptr(), bs, b, k, n, rows, m, 1 if center else 0, Wt.data_ptr(), out.data_ptr(), scratch.data_ptr(), pneed, st))
        raw = torch.cat([out[:72], state.to(torch.float64)]).cpu().numpy()          # the one host read: the header, the spectrum, the members' state
        head, sta = raw[:72], raw[72:].astype(np.int64)
        degenerate = np.nonzero(sta == 1)[0].tolist()
        domain = np.nonzero(sta == 2)[0].tolist()
        if check:
            if degenerate or (sta == 4).any():
                raise ValueError(f"{DEGENERATE}: indices {np.nonzero((sta == 1) | (sta == 4))[0].tolist()}")
            if domain:
                raise ValueError(f"basis {domain[0]} is outside the log map's domain at the base: its largest principal angle to the base exceeds "
                                 f"pi/2 - 1e-6 (choose another base, or drop the basis): indices {domain}")
        ok = sta == 0
        nv = int(ok.sum())
        fit = None
        Wt[m] = torch.from_numpy(ok / max(nv, 1)).to(dev)                            # the mean tangent
        if npar:
            if nv < 2:
                raise ValueError(f"the covariate fit needs at least 2 valid members, got {nv}")
            xv = x[ok]
            xbar = xv.mean(axis=0)
            xc = xv - xbar
            if np.linalg.matrix_rank(xc) < npar:
                raise ValueError(f"covariates: the centred design matrix of the {nv} valid members has rank {np.linalg.matrix_rank(xc)} < P = {npar}")
            xtx = xc.T @ xc
            coef = np.zeros((npar, b))
            coef[:, ok] = np.linalg.solve(xtx, xc.T)                                 # S_p = sum_i coef[p, i] L_i
            icpt = np.zeros(b)
            icpt[ok] = 1.0 / nv
            icpt -= xbar @ coef
            cd = torch.from_numpy(np.concatenate([coef, icpt[None]])).to(dev)
            Wt[m + 1:] = cd
            tz = torch.nan_to_num(T, nan=0.0)
            okd = torch.from_numpy(ok).to(dev)
            tz = tz * okd[:, None] * okd[None, :]
            sg = cd[:npar] @ tz @ cd[:npar].t()
            fit = torch.cat([sg.flatten(), tz.diagonal().sum()[None], tz.sum()[None]]).cpu().numpy()      # the covariate fit's host read
        L.check(lib.dpb_pga_combine(A.data_ptr() if stacked is A else stacked.data_ptr(), Wt.data_ptr(), rows, tangents.data_ptr(), bs, b, k, n, cap, rows,
                                    fscratch.data_ptr(), fneed, scratch.data_ptr(), pneed, st))
    variance = head[8:8 + m].copy()
    total = float(head[1])
    info = {"variance": variance, "total_variance": total, "explained": np.cumsum(variance) / total if total > 0 else np.zeros(m),
            "scores": out[72:72 + b * m].view(b, m), "residual": out[72 + b * m:], "mean_tangent_norm": float(head[2]), "theta": theta, "tangent_gram": T,
            "mean_tangent": tangents[m], "degenerate": degenerate, "domain": domain, "solver": PGA_ROUTES[int(head[3])], "valid_members": nv}
    if info["solver"] == "subspace":
        info["subspace_iterations"], info["subspace_converged"] = int(head[4]), int(head[5]) == 1
    if isinstance(base, str):
        info["iterations"], info["converged"] = minfo["iterations"], minfo["converged"]
        for key in ("flag_iterations", "flag_converged"):
            if key in minfo:
                info[key] = minfo[key]
    if npar:
        sg = fit[:npar * npar].reshape(npar, npar)
        centred = float(fit[-2] - fit[-1] / nv)                                      # tr(H T H) over the valid members
        info.update({"slopes": tangents[m + 1:m + 1 + npar], "intercept": tangents[m + 1 + npar], "slope_norm": np.sqrt(np.clip(np.diag(sg), 0.0, None)),
                     "r2": float(np.trace(sg @ xtx) / centred) if centred > 0 else 0.0})
    return Y, tangents[:m], info


def linear_assignment(cost: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The batched linear-assignment problem: cost [B, k, k] (or one [k, k]) float64 on the device -> (col_of_row [B, k] int32, total [B] float64), the
    permutation minimising sum_i cost[b, i, col_of_row[b, i]] and that sum (dpb_linear_assignment: shortest augmenting paths, one workgroup per
    problem, ties broken on the lowest column index -- a function of the matrix alone, bitwise the same alone and in a batch).  k <= 128.  A problem
    with a non-finite entry returns -1 / NaN and spoils no other.  No host sync."""
    lib = L.load()
    if not torch.is_tensor(cost) or not cost.is_cuda:
        raise ValueError("cost must be a tensor on a HIP device (there is no CPU path)")
    if cost.dtype != torch.float64:
        raise ValueError(f"cost must be float64, got {cost.dtype}")
    cost = cost.detach().contiguous()
    if cost.dim() == 2:
        cost = cost[None]
    if cost.dim() != 3 or cost.shape[1] != cost.shape[2] or cost.numel() == 0:
        raise ValueError(f"cost must be a stack of square matrices [B, k, k], got {tuple(cost.shape)}")
    b, k, _ = cost.shape
    if k > MAX_RANK:
        raise ValueError(f"k = {k} exceeds the size {MAX_RANK} the assignment solver supports")
    need = int(lib.dpb_linear_assignment_scratch_bytes(b, k))
    if need == 0:
        raise L.DpbError(f"dpb_linear_assignment does not take B = {b}, k = {k}")
    with torch.cuda.device(cost.device):
        st = C.c_void_p(torch.cuda.current_stream(cost.device).cuda_stream)
        scratch = torch.empty(need, dtype=torch.uint8, device=cost.device)
        col = torch.empty(b, k, dtype=torch.int32, device=cost.device)
        total = torch.empty(b, dtype=torch.float64, device=cost.device)
        L.check(lib.dpb_linear_assignment(cost.data_ptr(), b, k, col.data_ptr(), total.data_ptr(), scratch.data_ptr(), need, st))
    return col, total


HUNGARIAN_DISTANCES = {"1/cosine": 0, "cosine": 1}


def hungarian_mean(A: torch.Tensor, init: int = 0, distance: str = "1/cosine", max_sweeps: int = 20, anchor: Optional[torch.Tensor] = None,
                   max_bytes: Optional[int] = None, check: bool = True) -> Tuple[torch.Tensor, dict]:
    """The Hungarian-matched mean of the directions of A [B, k, N]: with xhat the rows scaled to unit length in fp64 and the anchor Y = xhat[init]
    (or ``anchor`` [k, N]), a sweep matches every basis's rows one to one to the anchor's by the assignment pi_b minimising
    sum_i d(<y_i, xhat_{b, pi_b(i)}>), d = 1 / max(|c|, 2^-40) ('1/cosine', the reference's call) or 1 - |c| ('cosine'), takes the sign of each
    matched overlap, and sets Y_i = normalise(sum_b sign_b(i) xhat_{b, pi_b(i)}), rounded to fp32 once; that Y is the next sweep's anchor.  Sweeps stop
    when no pi_b and no sign changed (``converged``) or after max_sweeps (1: the plain anchor-matched mean); '1/cosine' has no monotone objective, so
    not converging is reported, not raised.  See include/dpb.h (dpb_matched_mean) for the kernels and the limits; any float dtype is converted to
    contiguous fp32; k <= 128.

    Returns Y [k, N] fp32 with unit rows in the ANCHOR's order -- row i is the direction matched to anchor row i; the rows are not orthogonalised --
    and info: ``perm`` [B, k] int32 (pi_b(i)), ``sign`` [B, k] int32, ``cost`` [sweeps, B] float64 numpy (each sweep's assignment totals),
    ``sweeps``, ``converged``, ``changed`` (list: (b, i) entries that changed per sweep; the first counts all B k), ``weight`` [k] fp32 (the mean over
    b of |<y_i, xhat_{b, pi_b(i)}>| against the final Y) and ``degenerate`` (indices).  One host read per sweep.  check: raise ValueError naming the
    degenerate bases (a zero or non-finite row); False returns the NaNs.  Bitwise reproducible; perm[b] and sign[b] do not depend on the other bases
    of the stack given the same anchor."""
    lib = L.load()
    A = _stack(A, "A")
    b, k, n = A.shape
    if distance not in HUNGARIAN_DISTANCES:
        raise ValueError(f"distance must be one of {sorted(HUNGARIAN_DISTANCES)}, got {distance!r}")
    if k > MAX_RANK:
        raise ValueError(f"k = {k} rows per basis exceeds the rank {MAX_RANK} the Hungarian mean supports")
    init, max_sweeps = int(init), int(max_sweeps)
    if not 0 <= init < b:
        raise ValueError(f"init = {init} outside [0, B = {b})")
    if max_sweeps < 1:
        raise ValueError(f"max_sweeps = {max_sweeps} must be >= 1")
    if anchor is not None:
        anchor = _device_f32(anchor, "anchor").to(A.device)
        if tuple(anchor.shape) != (k, n):
            raise ValueError(f"anchor must be [k = {k}, N = {n}], got {tuple(anchor.shape)}")
    max_bytes = DEFAULT_MAX_BYTES if max_bytes is None else int(max_bytes)
    need = int(lib.dpb_matched_mean_scratch_bytes(b, k, n))
    if need == 0:
        raise L.DpbError(f"dpb_matched_mean does not take B = {b}, k = {k}, N = {n}")
    if need > max_bytes:
        raise ValueError(f"the Hungarian mean of B = {b} bases of k = {k} rows needs {need} bytes of device scratch, max_bytes is {max_bytes}")
    dist = HUNGARIAN_DISTANCES[distance]
    with torch.cuda.device(A.device):
        st = C.c_void_p(torch.cuda.current_stream(A.device).cuda_stream)
        scratch = torch.empty(need, dtype=torch.uint8, device=A.device)
        Y = [torch.empty(k, n, dtype=torch.float32, device=A.device) for _ in range(2)]      # (a sweep's output must not alias its anchor)
        perm = torch.full((b, k), -1, dtype=torch.int32, device=A.device)
        sign = torch.zeros(b, k, dtype=torch.int32, device=A.device)
        info_d = torch.empty(1 + 2 * b, dtype=torch.float64, device=A.device)
        costs, changed, converged, degenerate = [], [], False, []
        cur = anchor
        for s in range(max_sweeps):
            out = Y[s % 2]
            L.check(lib.dpb_matched_mean(A.data_ptr(), b, k, n, None if cur is None else cur.data_ptr(), init, dist, out.data_ptr(), perm.data_ptr(),
                                         sign.data_ptr(), info_d.data_ptr(), scratch.data_ptr(), need, st))
            raw = info_d.cpu().numpy()                                   # the one host read of the sweep
            cur = out
            costs.append(raw[1:1 + b].copy())
            changed.append(int(raw[0]))
            degenerate = np.nonzero(raw[1 + b:] != 0)[0].tolist()
            if degenerate:
                break
            if changed[-1] == 0:
                converged = True
                break
        if check and degenerate:
            raise ValueError(f"degenerate bases (a zero or non-finite row, in the basis or in the anchor): indices {degenerate}")
        # weight: |<y_i, xhat_{b, pi_b(i)}>| against the final Y, from the same exact overlaps and row norms
        G = torch.empty(k, b * k, dtype=torch.float64, device=A.device)
        ss = torch.empty(b * k + k, dtype=torch.float64, device=A.device)
        L.check(lib.dpb_cross_gram(cur.data_ptr(), A.data_ptr(), G.data_ptr(), k, b * k, n, st))
        L.check(lib.dpb_row_sumsq(A.data_ptr(), b * k, n, ss.data_ptr(), st))
        L.check(lib.dpb_row_sumsq(cur.data_ptr(), k, n, ss[b * k:].data_ptr(), st))
        c = G.view(k, b, k) / (ss[b * k:].sqrt()[:, None, None] * ss[:b * k].sqrt().view(1, b, k))
        picked = c.gather(2, perm.t().clamp(min=0).long()[:, :, None])[:, :, 0]          # [k, B]
        weight = picked.abs().mean(dim=1).to(torch.float32)
    info = {"perm": perm, "sign": sign, "cost": np.stack(costs), "sweeps": len(costs), "converged": converged, "changed": changed, "weight": weight,
            "degenerate": degenerate, "distance": distance}
    return cur, info


def subspace_angles(A: torch.Tensor, B: Optional[torch.Tensor] = None, max_bytes: Optional[int] = None) -> torch.Tensor:
    """Principal angles theta [Ba, Bb, k] in radians, descending per pair (the convention of scipy.linalg.subspace_angles), between the row spans of
    the bases of A [Ba, k, N] and B [Bb, k, N] (None: A against itself).  See subspace_angles_and_distance."""
    return subspace_angles_and_distance(A, B, max_bytes)[0]


def geodesic_distance(A: torch.Tensor, B: Optional[torch.Tensor] = None, max_bytes: Optional[int] = None) -> torch.Tensor:
    """Geodesic distance on the Grassmannian, dist [Ba, Bb] = ||theta||_2 over the principal angles of each pair.  See subspace_angles_and_distance."""
    return subspace_angles_and_distance(A, B, max_bytes)[1]


def _affinity_block(lib, b: int, c: int, k: int, r: int, n: int, max_bytes: int) -> int:
    """members per block of flag_affinity: the largest m whose call -- min(m, B) x min(m, C) -- keeps its scratch within max_bytes (at least 1)"""
    need = lambda m: int(lib.dpb_flag_affinity_scratch_bytes(min(m, b), k, min(m, c), r, n))
    lo, hi = 1, max(b, c)
    if need(hi) <= max_bytes:
        return hi
    while lo < hi:                                     # need() grows with m
        mid = (lo + hi + 1) // 2
        if need(mid) <= max_bytes:
            lo = mid
        else:
            hi = mid - 1
    return lo


def flag_affinity(A: torch.Tensor, Y: torch.Tensor, max_bytes: Optional[int] = None, check: bool = True) -> torch.Tensor:
    """The chordal affinity aff [B, C] (float64, on the device) between every basis of A [B, k, N] and every basis of Y [C, r, N], r smaller or larger
    than k: aff[i, c] = sum_j cos^2 theta_j(A_i, Y_c) = ||Q_Y Q_A^T||_F^2 in [0, min(r, k)] -- how much of a rank-r basis a rank-k one holds, where
    subspace_angles refuses unequal ranks; r - aff is the squared chordal distance flag_kmeans minimises (dpb_flag_affinity; include/dpb.h).  A [k, N]
    or [r, N] tensor is one basis; rows need not be orthonormal, only independent; any float dtype is converted to contiguous fp32; k, r <= 64.

    Entry (i, c) is bitwise a function of A_i, Y_c and N alone: the same alone, in any stack, and through the blocks of members a stack goes through
    when one call's scratch would exceed max_bytes.  check: raise ValueError naming the degenerate bases (a NaN row for one of A, a NaN column for
    one of Y; one host sync); False returns the NaNs and does not synchronise."""
    lib = L.load()
    A = _stack(A, "A")
    Y = _stack(Y, "Y").to(A.device)
    b, k, n = A.shape
    c, r = Y.shape[0], Y.shape[1]
    if Y.shape[2] != n:
        raise ValueError(f"A holds rows of length N = {n}, Y of N = {Y.shape[2]}: they must match")
    if k > FLAG_MEAN_MAX_RANK or r > FLAG_MEAN_MAX_RANK:
        raise ValueError(f"k = {k} or r = {r} rows per basis exceeds the rank {FLAG_MEAN_MAX_RANK} the affinity supports")
    if max(k, r) > n:
        raise ValueError(f"k = {k} or r = {r} rows per basis exceeds their length N = {n}: they cannot be independent")
    max_bytes = DEFAULT_MAX_BYTES if max_bytes is None else int(max_bytes)
    with torch.cuda.device(A.device):
        st = C.c_void_p(torch.cuda.current_stream(A.device).cuda_stream)
        blk = _affinity_block(lib, b, c, k, r, n, max_bytes)
        need = int(lib.dpb_flag_affinity_scratch_bytes(min(blk, b), k, min(blk, c), r, n))
        if need == 0:
            raise L.DpbError(f"dpb_flag_affinity does not take B = {b}, k = {k}, C = {c}, r = {r}, N = {n}")
        scratch = torch.empty(need, dtype=torch.uint8, device=A.device)
        aff = torch.empty(b, c, dtype=torch.float64, device=A.device)
        if blk >= max(b, c):
            L.check(lib.dpb_flag_affinity(A.data_ptr(), Y.data_ptr(), b, k, c, r, n, aff.data_ptr(), scratch.data_ptr(), need, st))
        else:
            for i0 in range(0, b, blk):
                i1 = min(i0 + blk, b)
                for j0 in range(0, c, blk):
                    j1 = min(j0 + blk, c)
                    part = torch.empty(i1 - i0, j1 - j0, dtype=torch.float64, device=A.device)
                    L.check(lib.dpb_flag_affinity(A[i0:i1].data_ptr(), Y[j0:j1].data_ptr(), i1 - i0, k, j1 - j0, r, n, part.data_ptr(),
                                                  scratch.data_ptr(), need, st))
                    aff[i0:i1, j0:j1] = part
    if check:
        bad = torch.isnan(aff)
        if bool(bad.any()):
            rows = bad.all(dim=1).nonzero().flatten().tolist()
            cols = bad.all(dim=0).nonzero().flatten().tolist()
            raise ValueError(f"{DEGENERATE}: indices {rows} of A, {cols} of Y")
    return aff


def _kmeans_state(scratch: torch.Tensor, host_bytes: int, b: int, c: int) -> dict:
    """the host part of a dpb_flag_kmeans_* block (include/dpb.h): one device read"""
    raw = scratch[:host_bytes].cpu().numpy()
    head = raw[:16].view(np.int32)
    ints = raw[32:].view(np.int32)
    return {"moved": int(head[0]), "kept": int(head[1]), "J": float(raw[16:24].view(np.float64)[0]), "sizes": ints[:c].copy(),
            "changed": ints[c:2 * c].copy(), "seeds": ints[2 * c:3 * c].copy(), "labels": ints[3 * c:3 * c + b].copy(),
            "flags": ints[3 * c + b:3 * c + 2 * b].copy()}


def flag_kmeans(A: torch.Tensor, n_clusters: int, rank: Optional[int] = None, init=0, max_rounds: int = 50, inner_iter: int = 200, tol: float = 1e-12,
                check_every: int = 16, seed: int = 0, max_bytes: Optional[int] = None, check: bool = True,
                history: bool = False, timings: bool = False) -> Tuple[torch.Tensor, torch.Tensor, dict]:
    """Flag k-means: the row spans of A [B, k, N] clustered into n_clusters = C families, each with a rank-``rank`` (None: k) flag mean as its centre --
    Lloyd's algorithm with r - flag_affinity as the distance.  The rank-r flag mean of a cluster maximises the summed affinity of its members, so the
    objective J = sum_i (r - a[i, label_i]) cannot rise (dpb_flag_kmeans_*; see include/dpb.h for the method and the limits).  k <= 64, 1 <= C <= B,
    1 <= rank <= k; rows need not be orthonormal, only independent; any float dtype is converted to contiguous fp32.

    Seeds: ``init`` is a member index -- each further seed is then the member whose smallest chordal distance^2 to the seeds so far is largest, the lowest
    index on a tie -- or a sequence of C distinct member indices.  Every member starts at its nearest seed.  A round fits every cluster's centre (flag_mean's
    solver on the cluster's part of the whitened Gram, at most inner_iter iterations to tol in chunks of check_every; a cluster whose member set did
    not change is not solved again), computes every member's affinity to every centre in one pass over the Gram, and moves member i to argmax_c a[i, c]
    (lowest c on a tie) if that exceeds its own by more than 1e-12 r; a cluster all of whose members want to leave keeps the one it holds best.  The
    run stops when no label changed or after max_rounds rounds; the centres and affinities of the final labels are always computed (max_rounds = 0
    labels by the seeds and fits once).  At the end the clusters are renumbered by their lowest member index.

    Returns labels [B] (int32, on the device), Y [C, rank, N] (fp32, orthonormal rows per centre in descending eigenvalue order) and info: ``rounds``,
    ``converged``, ``objective`` (fp64 numpy, one entry per fit, the start included), ``monotone`` (no entry rose by more than 1e-12 relative plus
    1e-15 B r), ``moved`` (per round), ``kept`` (how often the keep rule acted), ``sizes`` [C], ``weight`` [C, rank] (fp32: the mean cos^2 within the
    cluster), ``eigenvalues`` (per cluster: all Ritz values of its block), ``gap`` [C] (after row rank, or None), ``inner_iterations`` and
    ``inner_converged`` [C] (of each centre's last fit), ``affinity`` [B, C] (float64, on the device), ``seeds``, ``start`` (the start labels) and
    ``degenerate``; history=True adds ``history``: the labels after every round that moved a member, in the run's own numbering (cluster c grew from
    seed c); timings=True adds ``timings``: wall-clock ms of init, of every fit's update and assignment (the host read included) and of finish, with a
    device synchronisation at each boundary (a measuring aid: it adds host waits).  An inner solve or a run that does not converge, and monotone = False (which can follow from the former), are reported, not raised.
    check: raise ValueError naming the degenerate members; False gives them label -1 and NaN affinities and clusters the others.  One host read per
    round (and one per chunk of the inner solves).  Bitwise reproducible."""
    lib = L.load()
    A = _stack(A, "A")
    b, k, n = A.shape
    if k > FRECHET_MAX_RANK:
        raise ValueError(f"k = {k} rows per basis exceeds the rank {FRECHET_MAX_RANK} flag k-means supports")
    if k > n:
        raise ValueError(f"k = {k} rows per basis exceeds their length N = {n}: they cannot be independent")
    nc = int(n_clusters)
    if not 1 <= nc <= b:
        raise ValueError(f"n_clusters = {nc} outside [1, B = {b}]")
    r = k if rank is None else int(rank)
    if not 1 <= r <= k:
        raise ValueError(f"rank = {r} outside [1, k = {k}]")
    if isinstance(init, (int, np.integer)):
        seeds = [int(init)]
        if not 0 <= seeds[0] < b:
            raise ValueError(f"init = {seeds[0]} outside [0, B = {b})")
    else:
        seeds = [int(s) for s in init]
        if len(seeds) != nc or len(set(seeds)) != nc or any(s < 0 or s >= b for s in seeds):
            raise ValueError(f"init must be a member index or {nc} distinct member indices in [0, {b}), got {seeds}")
    max_rounds, inner_iter, check_every, seed = int(max_rounds), int(inner_iter), int(check_every), int(seed)
    if max_rounds < 0 or inner_iter < 0 or check_every < 1 or not tol >= 0 or seed < 0:
        raise ValueError(f"max_rounds = {max_rounds} and inner_iter = {inner_iter} must be >= 0, check_every = {check_every} >= 1, tol = {tol} >= 0 and "
                         f"seed = {seed} >= 0")
    max_bytes = DEFAULT_MAX_BYTES if max_bytes is None else int(max_bytes)
    need = int(lib.dpb_flag_kmeans_scratch_bytes(b, k, n, nc, r))
    host_bytes = int(lib.dpb_flag_kmeans_host_bytes(b, k, n, nc, r))
    if need == 0:
        raise L.DpbError(f"dpb_flag_kmeans does not take B = {b}, k = {k}, N = {n}, C = {nc}, r = {r}")
    if need > max_bytes:
        raise ValueError(f"flag k-means of B = {b} bases of k = {k} rows needs {need} bytes of device scratch (the fp64 Gram of all {b * k} rows), "
                         f"max_bytes is {max_bytes}")
    fits = {}                                            # cluster -> its last fit: (weight, info_d, members)
    with torch.cuda.device(A.device):
        st = C.c_void_p(torch.cuda.current_stream(A.device).cuda_stream)
        dev = A.device
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        times = {"init_ms": 0.0, "update_ms": [], "assign_ms": [], "finish_ms": 0.0}

        def lap(t0=None):
            if not timings:
                return 0.0
            torch.cuda.synchronize(dev)
            now = time.perf_counter()
            return now if t0 is None else (now - t0) * 1e3
        t0 = lap()
        L.check(lib.dpb_flag_kmeans_init(A.data_ptr(), b, k, n, nc, r, (C.c_int32 * len(seeds))(*seeds), len(seeds), scratch.data_ptr(), need, st))
        state = _kmeans_state(scratch, host_bytes, b, nc)
        times["init_ms"] = lap(t0)
        degenerate = np.nonzero(state["flags"] != 0)[0].tolist()
        if check and degenerate:
            raise ValueError(f"{DEGENERATE}: indices {degenerate}")
        if degenerate and (set(degenerate) & set(state["seeds"].tolist()) or nc > b - len(degenerate)):
            raise ValueError(f"{DEGENERATE}: indices {degenerate} leave no {nc} usable seeds (seeds {state['seeds'].tolist()})")
        start = state["labels"].copy()

        def fit(clusters, sizes):
            jobs, extra = [], 0
            for c in clusters:
                m = int(sizes[c])
                fneed = int(lib.dpb_flag_mean_solver_bytes(m, k, r, inner_iter))
                if fneed == 0:
                    raise L.DpbError(f"dpb_flag_mean does not take B = {m}, k = {k}, r = {r}, max_iter = {inner_iter} on a cluster's Gram")
                extra += fneed + 8 * (m * k) ** 2
                if need + extra > max_bytes:
                    raise ValueError(f"the centres of flag k-means need {extra} more bytes of device scratch (the clusters' parts of the Gram), "
                                     f"max_bytes is {max_bytes}")
                gc = torch.empty((m * k) ** 2, dtype=torch.float64, device=dev)
                fs = torch.empty(fneed, dtype=torch.uint8, device=dev)
                L.check(lib.dpb_flag_kmeans_gather(c, m, gc.data_ptr(), b, k, n, nc, r, scratch.data_ptr(), need, st))
                L.check(lib.dpb_flag_mean_init(None, gc.data_ptr(), m, k, n, r, seed, inner_iter, fs.data_ptr(), fneed, st))
                jobs.append((c, m, gc, fs, fneed))
            asked, active = 0, jobs
            while asked < inner_iter and active:
                steps = min(check_every, inner_iter - asked)
                for c, m, gc, fs, fneed in active:
                    L.check(lib.dpb_flag_mean_iterate(steps, float(tol), gc.data_ptr(), m, k, n, r, inner_iter, fs.data_ptr(), fneed, st))
                asked += steps
                done = torch.stack([j[3][:4].view(torch.int32) for j in active]).flatten().tolist()      # the one host read of the chunk
                active = [j for j, d in zip(active, done) if d == 0]
            for c, m, gc, fs, fneed in jobs:
                weight = torch.empty(r, dtype=torch.float32, device=dev)
                theta = torch.empty(m, r, dtype=torch.float32, device=dev)
                ct = torch.empty(m * k, r, dtype=torch.float64, device=dev)
                info_d = torch.empty(72 + m, dtype=torch.float64, device=dev)
                L.check(lib.dpb_flag_mean_finish(None, gc.data_ptr(), None, weight.data_ptr(), theta.data_ptr(), ct.data_ptr(), info_d.data_ptr(), m, k, n,
                                                 r, inner_iter, fs.data_ptr(), fneed, st))
                L.check(lib.dpb_flag_kmeans_set_centre(c, m, ct.data_ptr(), b, k, n, nc, r, scratch.data_ptr(), need, st))
                fits[c] = (weight, info_d, m)

        objective, moved, hist, kept, rounds, converged = [], [], [], 0, 0, False
        while True:
            t0 = lap()
            fit([c for c in range(nc) if state["changed"][c]], state["sizes"])
            times["update_ms"].append(lap(t0))
            t0 = lap()
            apply = rounds < max_rounds
            L.check(lib.dpb_flag_kmeans_assign(1 if apply else 0, b, k, n, nc, r, scratch.data_ptr(), need, st))
            state = _kmeans_state(scratch, host_bytes, b, nc)                                            # the one host read of the round
            times["assign_ms"].append(lap(t0))
            objective.append(state["J"])
            if not apply:
                break
            rounds += 1
            moved.append(state["moved"])
            kept += state["kept"]
            if state["moved"] == 0:
                converged = True
                break
            hist.append(state["labels"].copy())
        t0 = lap()
        Y = torch.empty(nc, r, n, dtype=torch.float32, device=dev)
        L.check(lib.dpb_flag_kmeans_finish(A.data_ptr(), Y.data_ptr(), b, k, n, nc, r, scratch.data_ptr(), need, st))
        times["finish_ms"] = lap(t0)
        off = int(lib.dpb_flag_kmeans_affinity(b, k, n, nc, r, scratch.data_ptr())) - scratch.data_ptr()
        aff = scratch[off:off + 8 * b * nc].view(torch.float64).view(b, nc).clone()
        raws = torch.cat([fits[c][1] for c in range(nc)]).cpu().numpy()
        # the clusters renumbered by their lowest member index
        labels_h = state["labels"]
        first = {}
        for i, c in enumerate(labels_h.tolist()):
            if c >= 0:
                first.setdefault(c, i)
        perm = sorted(first, key=first.get)
        inv = np.full(nc + 1, -1, dtype=np.int32)
        inv[perm] = np.arange(nc, dtype=np.int32)
        labels = torch.from_numpy(inv[labels_h]).to(dev)                                                  # (label -1 reads the last slot: -1)
        pidx = torch.tensor(perm, dtype=torch.long, device=dev)
        Y, aff = Y[pidx].contiguous(), aff[:, pidx].contiguous()
        weight = torch.stack([fits[c][0] for c in perm])
    eig, gap, inner_it, inner_ok, o = {}, {}, {}, {}, 0
    for c in range(nc):
        m = fits[c][2]
        raw = raws[o:o + 72 + m]
        o += 72 + m
        w = int(raw[3])
        eig[c] = raw[8:8 + w] / m
        gap[c] = float(eig[c][r - 1] - eig[c][r]) if w > r else None
        inner_it[c], inner_ok[c] = int(raw[0]), int(raw[1]) == 1
    objective = np.array(objective, dtype=np.float64)
    rise = objective[1:] - objective[:-1]
    info = {"rounds": rounds, "converged": converged, "objective": objective,
            "monotone": bool(np.all(rise <= 1e-12 * np.abs(objective[:-1]) + 1e-15 * b * r)), "moved": moved, "kept": kept,
            "sizes": np.array([int(state["sizes"][c]) for c in perm]), "weight": weight, "eigenvalues": [eig[c] for c in perm],
            "gap": [gap[c] for c in perm], "inner_iterations": [inner_it[c] for c in perm], "inner_converged": [inner_ok[c] for c in perm],
            "affinity": aff, "seeds": [int(state["seeds"][c]) for c in perm], "start": start, "degenerate": degenerate}
    if history:
        info["history"] = hist
    if timings:
        info["timings"] = times
    return labels, Y, info
