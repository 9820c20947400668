"""dpb_cgls_init / _h_step / _x_step and dpb_newton_residual / _update (csrc/cgls.hip) against the float64 restatement of tests/_cgls_ref.py.

The kernels know nothing of J: c, w0, q and w are whatever the caller hands them, so the tests hand them random rows.  Shapes: R = 1, 3, 257 rows
(257: the second launch group of 256), N = 5 (a ragged group of four), 4096 (exactly one slice), 4099 (a second slice, and rows that start at every
alignment), D = 7, 4097.  Every step is compared from the DEVICE's own previous state (the restatement is re-seeded with it), so a figure is the
error of one step: elements within one fp32 ulp (the same fp64 expression, whose scalar differs by the order of an fp64 sum), scalars within
max(N, D) 2^-52 relative, the bound of an fp64 sum of non-negative terms taken in another order.  On small-integer data with dyadic alpha and beta
every operation is exact in either precision and order: bitwise."""
import numpy as np
import pytest
import torch

import _cgls_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 5, 7), (3, 4096, 7), (3, 4099, 4097), (257, 5, 4097), (257, 4099, 7)]
MU_ABS, MU_REL = 0.03, 0.2


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return "cuda:0"


def _place(a, off=0):
    """the array on the device as a contiguous view that starts `off` floats into a fresh allocation"""
    a = np.ascontiguousarray(a, np.float32)
    buf = torch.zeros(a.size + off + 4, dtype=torch.float32, device=_dev())
    v = buf[off:off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == (4 * off) % 16
    return v


def _state(Rn, N, D, off=0):
    from diffusion_pullback_amd.engine import CglsState
    s = CglsState(Rn, N, D, _dev())
    s.delta, s.p, s.r = (_place(np.full(sh, 7.0, np.float32), off) for sh in ((Rn, N), (Rn, N), (Rn, D)))
    return s


def _rows(s):
    """the device state as a restatement seeded with it"""
    torch.cuda.synchronize()
    return R.Rows(s.delta.cpu().numpy().copy(), s.r.cpu().numpy().copy(), s.p.cpu().numpy().copy(), s.state.cpu().numpy().copy())


def _bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_rows(a, b):
    return _bits(a.delta, b.delta) and _bits(a.r, b.r) and _bits(a.p, b.p) and _bits(a.state, b.state)


def _gauss(Rn, N, D, seed):
    g = np.random.default_rng(seed)
    f = lambda *s: g.standard_normal(s).astype(np.float32)
    return dict(c=f(Rn, D), w0=f(Rn, N), q=[f(Rn, D), f(Rn, D)], w=[f(Rn, N), f(Rn, N)])


def _run(d, off=0, tol=0.0, mu_abs=MU_ABS, mu_rel=MU_REL, rounds=2, check=None):
    """init and `rounds` rounds on the device; check(name, device Rows before, device Rows after, device hist, inputs) after every step.  Returns
    the final Rows."""
    from diffusion_pullback_amd import engine as E
    Rn, D = d["c"].shape
    N = d["w0"].shape[1]
    s = _state(Rn, N, D, off)
    _, hist = E.cgls_init(_place(d["c"], off), _place(d["w0"], off), mu_abs, mu_rel, tol, into=s)
    cur = _rows(s)
    if check:
        check("init", None, cur, hist.cpu().numpy(), None)
    for i in range(rounds):
        hist = E.cgls_h_step(s, _place(d["q"][i], off))
        nxt = _rows(s)
        if check:
            check("h", cur, nxt, hist.cpu().numpy(), d["q"][i])
        cur = nxt
        hist = E.cgls_x_step(s, _place(d["w"][i], off), tol)
        nxt = _rows(s)
        if check:
            check("x", cur, nxt, hist.cpu().numpy(), d["w"][i])
        cur = nxt
    return cur


@pytest.mark.parametrize("Rn,N,D", SHAPES)
def test_gaussian_rows_against_float64(Rn, N, D):
    bar = max(N, D) * 2.0 ** -52
    close = lambda a, b: (np.abs(a - b) <= bar * np.abs(b)).all()
    ulp = lambda a, b: (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(b))).all()
    for off in (0, 1):
        d = _gauss(Rn, N, D, 10 * Rn + off)

        def check(name, before, after, hist, inp):
            if name == "init":
                ref, rh = R.init_ref(d["c"], d["w0"], MU_ABS, MU_REL, 0.0)
            else:
                ref = before.copy()
                rh = R.h_step_ref(ref, inp) if name == "h" else R.x_step_ref(ref, inp, 0.0)
            assert ulp(after.delta, ref.delta) and ulp(after.r, ref.r) and ulp(after.p, ref.p), (name, off)
            assert close(after.state, ref.state) and close(hist, rh), (name, off, np.abs(after.state - ref.state).max())
            assert (after.state[:, R.FLAG] == 0).all() and _bits(hist, after.state[:, [R.GAMMA, R.RR, R.DD, R.FLAG]])

        fin = _run(d, off, check=check)
        assert (fin.state[:, R.ITERS] == 2).all() and np.isfinite(fin.delta).all()


def _dyadic(Rn, N, D, seed):
    """w0 with four entries +-2 (gamma = ||p||^2 = 16) at both ends of the row, q with four entries +-1 (||q||^2 = 4), mu = 1/4: alpha = 16 / (4 + 4)
    = 2; s = w - mu delta has half-integers, gamma' a multiple of 1/4, beta = gamma' / 16 dyadic"""
    g = np.random.default_rng(seed)
    ints = lambda *s: g.integers(-8, 9, s).astype(np.float32)
    w0 = np.zeros((Rn, N), np.float32); q = np.zeros((Rn, D), np.float32)
    sg = lambda: g.choice(np.array([-1.0, 1.0], np.float32), size=Rn)
    for j in (0, 1, N - 2, N - 1):
        w0[:, j] = 2 * sg()
    for j in (0, 2, D - 3, D - 1):
        q[:, j] = sg()
    return dict(c=ints(Rn, D), w0=w0, q=[q], w=[ints(Rn, N)])


@pytest.mark.parametrize("Rn,N,D", SHAPES)
def test_small_integer_data_is_exact(Rn, N, D):
    for off in (0, 1):
        d = _dyadic(Rn, N, D, 7 * Rn + off)
        ref, _ = R.init_ref(d["c"], d["w0"], 0.25, 0.0, 0.0)

        def check(name, before, after, hist, inp):
            rh = ref.hist() if name == "init" else (R.h_step_ref(ref, inp) if name == "h" else R.x_step_ref(ref, inp, 0.0))
            assert _same_rows(after, ref) and _bits(hist, rh), (name, off)

        fin = _run(d, off, mu_abs=0.25, mu_rel=0.0, rounds=1, check=check)
        assert (fin.state[:, R.MU] == 0.25).all() and (fin.state[:, R.GAMMA0] == 16).all() and (fin.state[:, R.FLAG] == 0).all()
        assert _bits(fin.delta, 2 * d["w0"])                                   # alpha = 2


def test_a_row_is_the_same_alone_anywhere_in_a_stack_and_at_either_alignment():
    """N = 4099, D = 4097: the rows of a stack start at every alignment of a float4"""
    N, D = 4099, 4097
    d = _gauss(3, N, D, 3)
    stack = [_run(d, off) for off in (0, 1)]
    assert _same_rows(stack[0], stack[1])
    five = {k: (np.concatenate([v[::-1], v[:2]]) if not isinstance(v, list) else [np.concatenate([a[::-1], a[:2]]) for a in v]) for k, v in d.items()}
    moved = _run(five)                                                          # rows 2, 1, 0, 0, 1 of the stack
    for b in range(3):
        one = {k: (v[b:b + 1] if not isinstance(v, list) else [a[b:b + 1] for a in v]) for k, v in d.items()}
        for off in (0, 1, 2, 3):
            alone = _run(one, off)
            for k in ("delta", "r", "p", "state"):
                assert _bits(getattr(alone, k)[0], getattr(stack[0], k)[b]), (b, off, k)
        for at in ([2, 3], [1, 4], [0])[b]:
            for k in ("delta", "r", "p", "state"):
                assert _bits(getattr(moved, k)[at], getattr(stack[0], k)[b]), (b, at, k)


def test_frozen_rows_are_handed_through_bit_for_bit():
    """row 1 has J^T c = 0: frozen by init; tol = 10 then freezes every row at the first x-step; the second round (NaN inputs included) moves nothing"""
    from diffusion_pullback_amd import engine as E
    N, D = 4099, 4097
    d = _gauss(3, N, D, 5)
    d["w0"][1] = 0.0
    s = _state(3, N, D)
    _, h0 = E.cgls_init(_place(d["c"]), _place(d["w0"]), MU_ABS, MU_REL, 0.0, into=s)
    a = _rows(s)
    assert h0[:, 3].tolist() == [0.0, 1.0, 0.0] and _bits(a.delta[1], np.zeros(N, np.float32)) and _bits(a.r[1], d["c"][1]) and _bits(a.p[1], d["w0"][1])
    E.cgls_h_step(s, _place(d["q"][0]))
    h1 = E.cgls_x_step(s, _place(d["w"][0]), 10.0)
    b = _rows(s)
    assert h1[:, 3].tolist() == [1.0, 1.0, 1.0] and b.state[:, R.ITERS].tolist() == [1.0, 0.0, 1.0]
    for k in ("delta", "r", "p", "state"):
        assert _bits(getattr(b, k)[1], getattr(a, k)[1]), k
    junk_q, junk_w = d["q"][1].copy(), d["w"][1].copy()
    junk_q[0, 5] = np.nan; junk_w[2, 0] = np.inf
    h2 = E.cgls_h_step(s, _place(junk_q))
    h3 = E.cgls_x_step(s, _place(junk_w), 0.0)
    assert _same_rows(_rows(s), b) and torch.equal(h2, h1) and torch.equal(h3, h1)


def test_a_zero_denominator_freezes_the_row_with_flag_2():
    from diffusion_pullback_amd import engine as E
    d = _gauss(3, 5, 7, 8)
    d["q"][0][2] = 0.0
    s = _state(3, 5, 7)
    E.cgls_init(_place(d["c"]), _place(d["w0"]), 0.0, 0.0, 0.0, into=s)
    a = _rows(s)
    h = E.cgls_h_step(s, _place(d["q"][0]))
    b = _rows(s)
    assert h[:, 3].tolist() == [0.0, 0.0, 2.0]
    for k in ("delta", "r", "p"):
        assert _bits(getattr(b, k)[2], getattr(a, k)[2]), k
    E.cgls_x_step(s, _place(d["w"][0]), 0.0)
    c = _rows(s)
    assert all(_bits(getattr(c, k)[2], getattr(a, k)[2]) for k in ("delta", "r", "p")) and c.state[2, R.ITERS] == 0 and c.state[0, R.ITERS] == 1
    # c = 0 with a w0 that is not J^T c: no scale for mu_rel
    d["c"][1] = 0.0
    _, h = E.cgls_init(_place(d["c"]), _place(d["w0"]), 0.0, 0.1, 0.0, into=s)
    assert h[:, 3].tolist() == [0.0, 2.0, 0.0]


@pytest.mark.parametrize("where", ["c", "w0", "q", "p", "w"])
def test_a_non_finite_input_is_nan_in_exactly_that_row(where):
    N, D = 4099, 4097
    d = _gauss(3, N, D, 9)
    clean = _run(d, rounds=1)
    bad = {k: (v.copy() if not isinstance(v, list) else [a.copy() for a in v]) for k, v in d.items()}
    if where in ("c", "w0"):
        bad[where][1, -1] = np.nan
    elif where == "q":
        bad["q"][0][1, 4096] = np.inf
    elif where == "w":
        bad["w"][0][1, 4097] = np.nan
    if where != "p":
        got = _run(bad, rounds=1)
    else:                                                                       # p is the solver's own: poison it between init and the h-step
        from diffusion_pullback_amd import engine as E
        s = _state(3, N, D)
        E.cgls_init(_place(d["c"]), _place(d["w0"]), MU_ABS, MU_REL, 0.0, into=s)
        s.p[1, 17] = float("nan")
        E.cgls_h_step(s, _place(d["q"][0]))
        E.cgls_x_step(s, _place(d["w"][0]), 0.0)
        got = _rows(s)
    assert got.state[1, R.FLAG] == 3 and np.isnan(got.delta[1]).all() and np.isnan(got.r[1]).all() and np.isnan(got.p[1]).all()
    assert np.isnan(got.state[1, [R.GAMMA, R.RR, R.DD]]).all()
    for b in (0, 2):
        for k in ("delta", "r", "p", "state"):
            assert _bits(getattr(got, k)[b], getattr(clean, k)[b]), (b, k)


@pytest.mark.parametrize("n,D", [(1, 7), (3, 4097), (257, 7)])
def test_newton_residual(n, D):
    from diffusion_pullback_amd.engine import newton_residual
    g = np.random.default_rng(n + D)
    dirs = g.integers(0, 2, n).tolist(); signs = g.choice([-1.0, 1.0], n).tolist(); scale = g.choice([0.5, 2.0, 3.0], n).tolist()
    for kind, off in (("dyadic", 0), ("dyadic", 1), ("gauss", 0), ("gauss", 1)):
        draw = (lambda *s: g.integers(-8, 9, s).astype(np.float32)) if kind == "dyadic" else (lambda *s: g.standard_normal(s).astype(np.float32))
        h0, h, u = draw(n, D), draw(n, D), draw(2, D)
        frac = 0.75
        got = newton_residual(_place(h0, off), _place(h, off), _place(u, off), dirs, signs, scale, frac).cpu().numpy()
        ref = R.residual_ref(h0, h, u, dirs, signs, scale, frac)
        if kind == "dyadic":
            assert _bits(got, ref), off
        else:
            assert (np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= np.spacing(np.abs(ref))).all(), off


@pytest.mark.parametrize("n,N", [(1, 5), (3, 4099), (257, 4096)])
def test_newton_update(n, N):
    from diffusion_pullback_amd.engine import newton_update
    g = np.random.default_rng(n + N)
    x = g.standard_normal((n, N)).astype(np.float32); delta = g.standard_normal((n, N)).astype(np.float32)
    state = g.standard_normal((n, 8)) ** 2
    state[:, R.DD] = (delta.astype(np.float64) ** 2).sum(axis=1)
    state[:, R.FLAG] = g.integers(0, 3, n)
    radius_mid = float(np.sqrt(np.median(state[:, R.DD]))) if n > 1 else 0.5 * float(np.sqrt(state[0, R.DD]))
    for radius in (0.0, radius_mid, 1e6):
        for off in (0, 1):
            out, stats = newton_update(_place(x, off), _place(delta, off), torch.from_numpy(state).to(_dev()), radius)
            ro, rs = R.update_ref(x, delta, state, radius)
            assert (np.abs(out.cpu().numpy().astype(np.float64) - ro.astype(np.float64)) <= np.spacing(np.abs(ro))).all(), (radius, off)
            assert _bits(stats.cpu().numpy(), rs), (radius, off)
    assert (rs[:, 2] == 1.0).all()
    _, rs = R.update_ref(x, delta, state, radius_mid)
    assert (rs[:, 2] < 1.0).any()
