"""dpb_direction_step and dpb_shift_stats (csrc/chain.hip) against the float64 restatement of tests/_chain_ref.py.

Bars, from the definitions in include/dpb.h: v is formed in fp64 and rounded once, so |vk - v| <= 2^-24 |v| plus the fp64 rounding of the norm.
One rounding is 2^-53; 2^-48 is allowed instead, because the v compared against is formed here from NUMPY's sum of squares (pairwise) while the device
divides by its own (a chain of about 25 additions): the two norms differ by several of those roundings, not by one, and 2^-48 covers 32 of them --
immaterial beside 2^-24 either way.  x_out = fl32(x + step v) with that v: 2^-24 |x_out| + 2^-24 |step v| (+ 2^-48 of either); the statistics are fp64
sums of at most 12 289 terms in chains of a few dozen additions: 1e-12 relative; the kept count is exact.  A SEGA decision can
only flip for an element within rounding distance of its threshold: the data below have none within 1e-6 (relative) in the float64 reference --
asserted on the CPU -- so no element is left out of any comparison."""
import numpy as np
import pytest
import torch

import _chain_ref as R

pytestmark = pytest.mark.gpu

NS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 12289]
E24, E48 = 2.0 ** -24, 2.0 ** -48


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return "cuda:0"


def _rows(n, N, seed):
    """Gaussian rows; row 1 scaled by 1e-20 and row 2 by 1e+15 where the stack has them"""
    g = np.random.default_rng(seed)
    W = g.standard_normal((n, N)).astype(np.float32)
    x = g.standard_normal((n, N)).astype(np.float32)
    if n > 1:
        W[1] *= np.float32(1e-20)
    if n > 2:
        W[2] *= np.float32(1e15)
    step = (0.25 + g.random(n) * 2).astype(np.float32)
    if n > 3:
        step[3] = -step[3]
    return W, x, step


def _run(W, x, step, sigma, out=None):
    from diffusion_pullback_amd.engine import direction_step
    d = _dev()
    xo, vk, st = direction_step(torch.from_numpy(W).to(d), torch.from_numpy(x).to(d) if out is None else out, step.tolist(), sigma, out=out)
    return xo.cpu().numpy(), vk.cpu().numpy(), st.cpu().numpy()


def _check(W, x, step, sigma, got):
    xo, vk, st = got
    xr, vr, sr, margin = R.direction_step_ref(W, x, step, sigma)
    n, N = W.shape
    assert margin.min() > 1e-6, "the float64 reference itself has an element at its SEGA threshold: pick another seed"
    for b in range(n):
        w = W[b].astype(np.float64)
        # std is sqrt of 1 - S1^2 / (N S2), a difference that cancels when the row is nearly constant: the 1e-12 bar on it needs a row that is not
        assert N < 2 or sigma <= 0 or 1.0 - w.sum() ** 2 / (N * sr[b, 0]) > 1e-3, "a nearly constant row: pick another seed"
        v = -w / np.sqrt(sr[b, 0])
        v[vr[b] == 0] = 0.0                                       # the rule's decisions (and exact zeros of w)
        assert st[b, 3] == 0 and st[b, 2] == sr[b, 2], (b, st[b], sr[b])
        assert abs(st[b, 0] - sr[b, 0]) <= 1e-12 * sr[b, 0] and abs(st[b, 1] - sr[b, 1]) <= 1e-12 * sr[b, 1], (b, st[b], sr[b])
        assert np.array_equal(vk[b] == 0, vr[b] == 0), b
        assert np.all(np.abs(vk[b] - v) <= (E24 + E48) * np.abs(v)), (b, np.abs(vk[b] - v).max())
        want = x[b].astype(np.float64) + np.float64(step[b]) * v
        bar = (E24 + E48) * (np.abs(xo[b].astype(np.float64)) + np.abs(np.float64(step[b]) * v))
        assert np.all(np.abs(xo[b] - want) <= bar), (b, (np.abs(xo[b] - want) - bar).max())


@pytest.mark.parametrize("N", NS)
def test_direction_step_against_float64(N):
    """n = 1 .. 5 rows (Gaussian, one scaled by 1e-20, one by 1e+15, one negative step), SEGA off and on at sigma = 0.5, 1, 2"""
    for n in range(1, 6):
        W, x, step = _rows(n, N, 1000 * N + n)
        for sigma in (0.0, 0.5, 1.0, 2.0):
            _check(W, x, step, sigma, _run(W, x, step, sigma))


def test_n_equal_one_keeps_its_element_under_sega():
    W = np.array([[3.0], [-2.0]], np.float32)
    xo, vk, st = _run(W, np.ones((2, 1), np.float32), np.array([0.5, 0.5], np.float32), 1.0)
    assert vk[:, 0].tolist() == [-1.0, 1.0] and xo[:, 0].tolist() == [0.5, 1.5] and st[:, 1:].tolist() == [[0, 1, 0], [0, 1, 0]]


@pytest.mark.parametrize("sigma", [0.0, 1.0])
def test_a_zero_row_and_an_inf_row_flag_themselves_and_nothing_else(sigma):
    """NaN and the flag in exactly that row of vk and x_out; every other row is bitwise that of the call without it"""
    for N in (5, 257, 4097):
        W, x, step = _rows(5, N, 77 + N)
        ref = _run(W, x, step, sigma)
        for bad_row, fill in ((1, 0.0), (3, np.inf), (0, np.nan)):
            Wb = W.copy()
            if fill == 0.0:
                Wb[bad_row] = 0
            else:
                Wb[bad_row, N // 2] = fill
            xo, vk, st = _run(Wb, x, step, sigma)
            assert st[:, 3].tolist() == [float(b == bad_row) for b in range(5)]
            assert np.isnan(xo[bad_row]).all() and np.isnan(vk[bad_row]).all() and st[bad_row, 1] == 0 and st[bad_row, 2] == 0
            keep = [b for b in range(5) if b != bad_row]
            for got, want in zip((xo, vk, st), ref):
                assert np.array_equal(got[keep], want[keep])
        # the call after a flagged one is unaffected (the scratch and the statistics carry nothing over)
        again = _run(W, x, step, sigma)
        assert all(np.array_equal(a, b) for a, b in zip(again, ref))


@pytest.mark.parametrize("N", [3, 5, 63, 257, 4097, 12289])
def test_a_row_is_bitwise_the_same_alone_and_anywhere_in_a_stack(N):
    """rows start at b N floats: for these N a row is 16-byte aligned at some positions and not at others"""
    W, x, step = _rows(5, N, 31 + N)
    for sigma in (0.0, 1.0):
        xo, vk, st = _run(W, x, step, sigma)
        for b in range(5):
            a = _run(W[b:b + 1], x[b:b + 1], step[b:b + 1], sigma)
            assert np.array_equal(a[0][0], xo[b]) and np.array_equal(a[1][0], vk[b]) and np.array_equal(a[2][0], st[b]), (N, b)
        p = np.array([3, 0, 4, 1, 2])
        xo2, vk2, st2 = _run(W[p], x[p], step[p], sigma)
        assert np.array_equal(xo2, xo[p]) and np.array_equal(vk2, vk[p]) and np.array_equal(st2, st[p])


def test_x_out_may_alias_x():
    for N in (5, 4096, 4097):
        W, x, step = _rows(4, N, 5 + N)
        ref = _run(W, x, step, 1.0)
        xt = torch.from_numpy(x.copy()).to(_dev())
        got = _run(W, x, step, 1.0, out=xt)
        assert all(np.array_equal(a, b) for a, b in zip(got, ref)) and np.array_equal(xt.cpu().numpy(), ref[0])


@pytest.mark.parametrize("D", NS)
def test_shift_stats_against_float64(D):
    """(<h - h0, c> / ||c||, ||h - h0||^2) within 1e-12 relative of float64, for n = 1 .. 5 rows, several directions, both signs and a scaled sign.
    The first is a sum of terms of both signs: the data are asserted, on the CPU, not to cancel by more than a factor of 1000 (sum |d c| against
    |sum d c|), so that a few dozen fp64 roundings of the terms stay far inside 1e-12 of the value."""
    from diffusion_pullback_amd.engine import shift_stats
    d = _dev()
    for n in range(1, 6):
        g = np.random.default_rng(9 * D + n)
        h0 = g.standard_normal((n, D)).astype(np.float32)
        h = (h0 + 0.01 * g.standard_normal((n, D))).astype(np.float32)
        u = g.standard_normal((3, D)).astype(np.float32)
        dirs = g.integers(0, 3, n).tolist()
        signs = [(1.0, -1.0, 0.5, -3.0, 1.0)[b] for b in range(n)]
        got = shift_stats(torch.from_numpy(h).to(d), torch.from_numpy(h0).to(d), torch.from_numpy(u).to(d), dirs, signs).cpu().numpy()
        ref = R.shift_stats_ref(h, h0, u, dirs, signs)
        for b in range(n):
            dd = h[b].astype(np.float64) - h0[b].astype(np.float64)
            c = signs[b] * u[dirs[b]].astype(np.float64)
            assert np.abs(dd * c).sum() <= 1e3 * abs((dd * c).sum()), "the terms of <h - h0, c> cancel: pick another seed"
            assert abs(got[b, 0] - ref[b, 0]) <= 1e-12 * abs(ref[b, 0]), (n, b, got[b], ref[b])
            assert abs(got[b, 1] - ref[b, 1]) <= 1e-12 * ref[b, 1], (n, b, got[b], ref[b])
        same = shift_stats(torch.from_numpy(h).to(d), torch.from_numpy(h).to(d), torch.from_numpy(u).to(d), dirs, signs).cpu().numpy()
        assert np.array_equal(same, np.zeros((n, 2)))             # a state against itself: exactly (0, 0)
