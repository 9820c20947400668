"""geometry.flag_affinity (dpb_flag_affinity, csrc/flagkmeans.hip) on the GPU against tests/_flag_kmeans_ref.py, the numpy float64 reference in the
ambient space (QR per basis, ||Q_a Q_y^T||_F^2), on the same fp32 inputs.

Bar, per entry: 4 2^-24 min(r, k), the project's bar for cos^2-like quantities (every cos^2 is formed from exact fp32 products accumulated in fp64; what
is left is the fp32 rounding of the inputs' own representation, which both sides share, times the whitening's condition)."""
import functools

import numpy as np
import pytest
import torch

import _flag_kmeans_ref as K
import _frechet_ref as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 4 * 2.0 ** -24

# (B, k, C, r, N)
SHAPES = [(1, 1, 1, 1, 5), (7, 5, 3, 2, 131), (5, 3, 4, 7, 40), (33, 2, 2, 2, 40), (3, 64, 2, 64, 4099), (40, 32, 5, 10, 2050)]


def _geo():
    from diffusion_pullback_amd import geometry
    return geometry


def _lib():
    from diffusion_pullback_amd import lib
    return lib.load()


def _dev(a):
    return torch.tensor(np.asarray(a), device=DEV)


@functools.lru_cache(maxsize=None)
def _case(b, k, c, r, n):
    """A: mixed at condition up to ~100 and row-scaled; Y: bases that share part of their span with members of A (so the entries spread over [0, min(r, k)])"""
    rng = np.random.default_rng(1000 * b + 10 * k + r)
    a = np.stack([np.diag(10.0 ** rng.uniform(-1, 1, k)) @ F.mixing(rng, k, 100.0 if i % 2 else 3.0) @ rng.standard_normal((k, n)) / np.sqrt(n)
                  for i in range(b)])
    y = []
    for j in range(c):
        rows = rng.standard_normal((r, n)) / np.sqrt(n)
        s = min(r, k) // 2 + (j % 2)
        rows[:s] = (a[j % b][:s] / np.linalg.norm(a[j % b][:s], axis=1, keepdims=True)) + 0.3 * rows[:s]
        y.append(F.mixing(rng, r, 30.0) @ rows)
    a, y = a.astype(np.float32), np.stack(y).astype(np.float32)
    a.setflags(write=False); y.setflags(write=False)
    return a, y, K.affinity_ref(a, y)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(str(x) for x in s))
def test_affinity_matches_the_reference(shape):
    b, k, c, r, n = shape
    a, y, ref = _case(*shape)
    aff = _geo().flag_affinity(_dev(a), _dev(y))
    assert aff.dtype == torch.float64 and tuple(aff.shape) == (b, c) and aff.is_cuda
    got = aff.cpu().numpy()
    err = np.abs(got - ref).max()
    print(f"{shape}: worst |aff - ref| {err:.2e} (bar {EPS * min(r, k):.2e}), range [{ref.min():.3f}, {ref.max():.3f}]")
    assert err <= EPS * min(r, k)
    assert (got >= -EPS).all() and (got <= min(r, k) + EPS * min(r, k)).all()


def test_angles_zero_small_and_right():
    """pairs at angle 0, 1e-4 and pi/2 (rank 3 against rank 2): sum cos^2 = 2, 2 - ~1e-8 and 0"""
    rng = np.random.default_rng(5)
    f = F.random_orthonormal(rng, 7, 260)
    a = f[:3]
    ys = [f[:2], np.stack([np.cos(1e-4) * f[0] + np.sin(1e-4) * f[3], f[1]]), f[4:6]]
    a32, y32 = a.astype(np.float32), np.stack(ys).astype(np.float32)
    ref = K.affinity_ref(a32[None], y32)
    got = _geo().flag_affinity(_dev(a32), _dev(y32)).cpu().numpy()
    print(f"angles 0, 1e-4, pi/2: got {got.tolist()}, ref {ref.tolist()}, worst {np.abs(got - ref).max():.2e}")
    assert np.abs(got - ref).max() <= EPS * 2
    assert abs(got[0, 0] - 2.0) <= EPS * 2 and abs(got[0, 2]) <= EPS * 2 and abs((2.0 - got[0, 1]) - np.sin(1e-4) ** 2) <= EPS * 2


def test_an_entry_is_bitwise_the_same_alone_in_a_stack_and_through_blocks():
    shape = (7, 5, 3, 2, 131)
    a, y, _ = _case(*shape)
    g = _geo()
    A, Y = _dev(a), _dev(y)
    full = g.flag_affinity(A, Y)
    alone = g.flag_affinity(A[4], Y[1])
    assert tuple(alone.shape) == (1, 1) and torch.equal(alone[0, 0], full[4, 1])
    part = g.flag_affinity(A[[6, 4, 0]], Y[[2, 1]])
    assert torch.equal(part, full[[6, 4, 0]][:, [2, 1]])
    small = int(_lib().dpb_flag_affinity_scratch_bytes(2, 5, 2, 2, 131))
    blocks = g.flag_affinity(A, Y, max_bytes=small)
    assert torch.equal(blocks, full)


def test_degenerate_bases_give_a_nan_row_and_column():
    shape = (7, 5, 3, 2, 131)
    a, y, ref = _case(*shape)
    a, y = a.copy(), y.copy()
    a[2, 1] = a[2, 0] * 2.0                     # dependent rows
    y[1, 0] = 0.0                               # a zero row
    g = _geo()
    aff = g.flag_affinity(_dev(a), _dev(y), check=False).cpu().numpy()
    bad = np.isnan(aff)
    assert bad[2].all() and bad[:, 1].all() and bad.sum() == 3 + 7 - 1
    ok = ~bad
    assert np.abs(aff[ok] - ref[ok]).max() <= EPS * 2
    with pytest.raises(ValueError, match=r"indices \[2\] of A, \[1\] of Y"):
        g.flag_affinity(_dev(a), _dev(y))
