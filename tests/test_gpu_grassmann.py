"""geometry.principal_vectors / grassmann_log / grassmann_geodesic / grassmann_exp (dpb_grassmann_pair / dpb_grassmann_exp, csrc/geodesic.hip) on the GPU
against tests/_grassmann_ref.py, the numpy float64 textbook restatement, computed on the host from the SAME fp32 inputs.

Bars:
 1. theta against scipy.linalg.subspace_angles: 1e-6 rad per angle (the bar of test_gpu_subspace_angles.py);
 2. theta against geometry.subspace_angles on the same inputs: 1e-6 rad;
 3. the span of every Y[d, j] (geodesic and exp), of Pa and of Pb against the reference span: largest principal angle, by scipy in float64, <= 1e-6 rad
    (the bar of test_gpu_frechet.py).  Worst seen on an MI355X: see WORST below;
 4. Pa Pa^T, Pb Pb^T, Y Y^T against I and Pa Pb^T against diag(cos theta): max abs <= 4 2^-24 in float64 on the host -- each stored row is an
    orthonormal fp64 row rounded once, so a Gram entry moves by at most 2 2^-24; the factor 2 is the margin;
 5. log: |H P^T| <= 4 2^-24 ||h_i|| + 1e-12 (row i), ||h_i|| against theta_i at the angle bar 1e-6, and for N <= 1000 the operator H^T (P P^T)^-1 P
    against the reference operator U Theta V^T Y0^T, Frobenius norm relative to max(1, ||Delta_ref||_F), <= 1e-6;
 6. exp: bar 3 against the exp reference on the (P, H) of grassmann_log at t = 1 and 0.5 and on a random (not horizontal) H of row norm ~sqrt(N) with a
    row-scaled P at t = 0.3; sigma against the reference singular values at 1e-6 relative, |sigma - ref| <= 1e-6 ref + 2^-24 sigma_max.  The floor is
    the precision of the tangent's own format: rounding H to fp32 moves every singular value by up to 2^-24 ||H|| (Weyl), so a value below that is
    rounding noise of the stored H (the theta = 0 rows of a log map, where the spans intersect) and has no relative accuracy to ask for: such a row
    is as much inside span P as orthogonal to it, and its horizontal part is a difference of two equal Gram terms;
 7. bitwise: a pair alone, at positions 0 and 2 of a stack of 3 and broadcast gives identical bits in every output; two runs are identical;
 8. refusals: the cut locus, a zero row, k = 65, the scratch-size entry.

Inputs: orthonormal 2k-frames with planted angles (all 1e-6; mixed {0, 1e-6, 1e-4, 1e-2, 0.3, 1.0, pi/2 - 1e-3}; spread up to pi/2 - 1e-3; uniform in
[0, 1.5]), as they are, with rows scaled by logspace(0, 2), and with rows mixed at condition 10 -- the three variants are the D = 3 stack of a call --
and intersecting spans (2k > N) from random rows.  A general mixing of condition 100 is left out on purpose: the Gram route loses
sqrt(eps cond^2) at theta -> 0 (4e-7 .. 2e-6 rad against scipy for the method itself, measured on the host).

WORST (MI355X, over every case below): spans of the geodesic's points 4.0e-8 rad, of the exp map's 4.3e-8, of the principal vectors 3.7e-8; exp(log) against
the geodesic 7.4e-8; theta against scipy 2.0e-7 (identical to subspace_angles); Gram entries 8.3e-8 (bar 2.4e-7); log operator 2.8e-8; sigma 0.28 of its bound."""
import functools

import numpy as np
import pytest
import torch

import _grassmann_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 1e-6
ORTH = 4 * 2.0 ** -24
TS = [-0.5, 0.0, 0.25, 0.5, 1.0, 1.5]
PLANTED = [(1, 7), (2, 5), (5, 67), (16, 64), (17, 259), (33, 4099), (64, 128), (64, 1000)]
INTERSECTING = [(5, 7), (16, 20), (64, 100)]
SETS = ["tiny", "mixed", "spread", "random"]
SHAPES = PLANTED + INTERSECTING


@pytest.fixture(autouse=True)
def _one_blas_thread():
    """the host references are hundreds of small QR / SVD calls: a threaded BLAS spends them waiting for its own pool"""
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        yield
        return
    with threadpool_limits(1):
        yield


def _np(t):
    return t.detach().cpu().numpy()


def _call(name, *arrays, **kw):
    """geometry.<name> on device copies of the numpy inputs; numpy outputs"""
    from diffusion_pullback_amd import geometry
    args = [torch.tensor(np.asarray(a), device=DEV) if isinstance(a, np.ndarray) else a for a in arrays]
    out = getattr(geometry, name)(*args, **kw)
    return tuple(_np(o) for o in out) if isinstance(out, tuple) else _np(out)


@functools.lru_cache(maxsize=None)
def _stacks(k, n):
    """the calls of a shape: a list of (label, A [D, k, N], B [D, k, N]) fp32, read-only"""
    out = []
    if (k, n) in PLANTED:
        for si, name in enumerate(SETS):
            rng = np.random.default_rng(100000 * si + 1000 * k + n)
            pairs = [R.family(rng, k, n, name, v) for v in range(3)]
            out.append((name, np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])))
        out.append(("random D=1", out[3][1][:1].copy(), out[3][2][:1].copy()))
    else:
        a, b = R.random_pair(k, n)
        rng = np.random.default_rng(5 * k + n)
        a3 = np.stack([a, R.scale_rows(rng, a.astype(np.float64)).astype(np.float32), R.mix_rows(rng, a.astype(np.float64)).astype(np.float32)])
        b3 = np.stack([b, R.scale_rows(rng, b.astype(np.float64)).astype(np.float32), R.mix_rows(rng, b.astype(np.float64)).astype(np.float32)])
        out += [("intersecting", a3, b3), ("intersecting D=1", a3[:1].copy(), b3[:1].copy())]
    for _, a, b in out:
        a.setflags(write=False)
        b.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _theta_ref(k, n):
    """scipy's angles of every pair of every call of the shape, descending, float64"""
    ref = [np.stack([R.angles_to(a[d], b[d]) for d in range(len(a))]) for _, a, b in _stacks(k, n)]
    for r in ref:
        r.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _geodesic_ref(k, n):
    ref = [np.stack([R.geodesic(a[d], b[d], TS) for d in range(len(a))]) for _, a, b in _stacks(k, n)]
    for r in ref:
        r.setflags(write=False)
    return ref


def _orth_err(y):
    y = y.astype(np.float64)
    return float(np.abs(y @ y.T - np.eye(len(y))).max())


@pytest.mark.parametrize("k,n", SHAPES)
def test_principal_vectors(k, n):
    worst = dict(scipy=0.0, angles=0.0, span=0.0, orth=0.0, cross=0.0)
    for (label, a, b), th_ref in zip(_stacks(k, n), _theta_ref(k, n)):
        pa, pb, theta = _call("principal_vectors", a, b)
        assert pa.shape == a.shape and pb.shape == b.shape and theta.shape == (len(a), k) and pa.dtype == np.float32 and theta.dtype == np.float32
        th_lib = _call("subspace_angles", a, b)
        for d in range(len(a)):
            worst["scipy"] = max(worst["scipy"], np.abs(theta[d] - th_ref[d]).max())
            worst["angles"] = max(worst["angles"], np.abs(theta[d].astype(np.float64) - th_lib[d, d]).max())
            worst["span"] = max(worst["span"], R.max_angle(pa[d], a[d]), R.max_angle(pb[d], b[d]))
            worst["orth"] = max(worst["orth"], _orth_err(pa[d]), _orth_err(pb[d]))
            cross = pa[d].astype(np.float64) @ pb[d].astype(np.float64).T
            worst["cross"] = max(worst["cross"], np.abs(cross - np.diag(np.cos(th_ref[d]))).max())
            assert (np.diff(theta[d]) <= 0).all(), (label, d)
    print(f"principal_vectors k={k} N={n}: theta vs scipy {worst['scipy']:.2e}, vs subspace_angles {worst['angles']:.2e}, spans {worst['span']:.2e} rad; "
          f"|P P^T - I| {worst['orth']:.2e}, |Pa Pb^T - diag cos| {worst['cross']:.2e} (bar {ORTH:.2e})")
    assert worst["scipy"] <= BAR and worst["angles"] <= BAR and worst["span"] <= BAR
    assert worst["orth"] <= ORTH and worst["cross"] <= ORTH


@pytest.mark.parametrize("k,n", SHAPES)
def test_geodesic(k, n):
    worst = dict(span=0.0, orth=0.0, theta=0.0)
    for (label, a, b), th_ref, y_ref in zip(_stacks(k, n), _theta_ref(k, n), _geodesic_ref(k, n)):
        y, theta = _call("grassmann_geodesic", a, b, TS)
        assert y.shape == (len(a), len(TS), k, n) and y.dtype == np.float32
        worst["theta"] = max(worst["theta"], np.abs(theta - th_ref).max())
        for d in range(len(a)):
            for j in range(len(TS)):
                worst["span"] = max(worst["span"], R.max_angle(y[d, j], y_ref[d, j]))
                worst["orth"] = max(worst["orth"], _orth_err(y[d, j]))
            assert R.max_angle(y[d, 1], a[d]) <= BAR and R.max_angle(y[d, 4], b[d]) <= BAR, (label, d)      # t = 0 and t = 1: the two ends
    print(f"grassmann_geodesic k={k} N={n}: spans vs the textbook geodesic {worst['span']:.2e} rad, theta {worst['theta']:.2e}, |Y Y^T - I| {worst['orth']:.2e}")
    assert worst["span"] <= BAR and worst["theta"] <= BAR
    assert worst["orth"] <= ORTH
    one = _call("grassmann_geodesic", _stacks(k, n)[0][1], _stacks(k, n)[0][2], 0.5)[0]                      # a float ts: T = 1
    assert one.shape == (len(_stacks(k, n)[0][1]), 1, k, n)


@pytest.mark.parametrize("k,n", SHAPES)
def test_log(k, n):
    worst = dict(horiz=0.0, norm=0.0, op=0.0, orth=0.0)
    for (label, a, b), th_ref in zip(_stacks(k, n), _theta_ref(k, n)):
        p, h, theta = _call("grassmann_log", a, b)
        for d in range(len(a)):
            p64, h64 = p[d].astype(np.float64), h[d].astype(np.float64)
            hn = np.linalg.norm(h64, axis=1)
            excess = np.abs(h64 @ p64.T).max(axis=1) - (ORTH * hn + 1e-12)
            worst["horiz"] = max(worst["horiz"], excess.max())
            worst["norm"] = max(worst["norm"], np.abs(hn - th_ref[d]).max())
            worst["orth"] = max(worst["orth"], _orth_err(p[d]))
            assert R.max_angle(p[d], a[d]) <= BAR, (label, d)
            assert abs(np.linalg.norm(h64) - np.linalg.norm(th_ref[d])) <= BAR * np.sqrt(k), (label, d)          # ||H||_F: the geodesic distance
            if n <= 1000:
                ref = R.log_operator(a[d], b[d])
                scale = max(1.0, float(np.linalg.norm(np.tan(th_ref[d]))))                                          # ||Delta_ref||_F = ||tan theta||_2
                worst["op"] = max(worst["op"], np.linalg.norm(R.tangent_operator(p64, h64) - ref) / scale)
    print(f"grassmann_log k={k} N={n}: |H P^T| above its bound by {worst['horiz']:.2e} (<= 0 passes), | ||h_i|| - theta_i | {worst['norm']:.2e}, "
          f"operator {worst['op']:.2e}, |P P^T - I| {worst['orth']:.2e}")
    assert worst["horiz"] <= 0.0
    assert worst["norm"] <= BAR and worst["op"] <= BAR
    assert worst["orth"] <= ORTH


def _sigma_err(s, s_ref):
    """largest |sigma - sigma_ref| in units of its bound 1e-6 sigma_ref + 2^-24 sigma_max (bar 6 of the module docstring)"""
    s = s.astype(np.float64)
    return float((np.abs(s - s_ref) / (1e-6 * s_ref + 2.0 ** -24 * s_ref.max() + 1e-300)).max())


@pytest.mark.parametrize("k,n", SHAPES)
def test_exp(k, n):
    worst = dict(span=0.0, sigma=0.0, orth=0.0, arrive=0.0)
    ts = [1.0, 0.5]
    for (label, a, b), y_geo in zip(_stacks(k, n), _geodesic_ref(k, n)):
        p, h, _ = _call("grassmann_log", a, b)
        y, sigma = _call("grassmann_exp", p, h, ts)
        assert y.shape == (len(a), 2, k, n) and sigma.shape == (len(a), k)
        for d in range(len(a)):
            y_ref, s_ref = R.exp_map(p[d], h[d], ts)
            worst["sigma"] = max(worst["sigma"], _sigma_err(sigma[d], s_ref))
            for j in range(2):
                worst["span"] = max(worst["span"], R.max_angle(y[d, j], y_ref[j]))
                worst["orth"] = max(worst["orth"], _orth_err(y[d, j]))
            # exp of the log reproduces the geodesic as a subspace: t = 1 is slice 4 of TS, t = 0.5 slice 3
            worst["arrive"] = max(worst["arrive"], R.max_angle(y[d, 0], y_geo[d, 4]), R.max_angle(y[d, 1], y_geo[d, 3]))
            assert (np.diff(sigma[d]) <= 0).all(), (label, d)
    # a random, not horizontal H of row norm ~sqrt(N) on a row-scaled P
    _, a, _ = _stacks(k, n)[0]
    rng = np.random.default_rng(31 * k + n)
    p = np.stack([R.scale_rows(rng, x.astype(np.float64)).astype(np.float32) for x in a])
    h = rng.standard_normal(p.shape).astype(np.float32)
    y, sigma = _call("grassmann_exp", p, h, [0.3])
    for d in range(len(p)):
        y_ref, s_ref = R.exp_map(p[d], h[d], [0.3])
        worst["sigma"] = max(worst["sigma"], _sigma_err(sigma[d], s_ref))
        worst["span"] = max(worst["span"], R.max_angle(y[d, 0], y_ref[0]))
        worst["orth"] = max(worst["orth"], _orth_err(y[d, 0]))
    print(f"grassmann_exp k={k} N={n}: spans vs the textbook exp {worst['span']:.2e} rad, exp(log) vs the geodesic {worst['arrive']:.2e} rad, "
          f"sigma at {worst['sigma']:.2e} of its bound, |Y Y^T - I| {worst['orth']:.2e}")
    assert worst["span"] <= BAR and worst["arrive"] <= BAR
    assert worst["sigma"] <= 1.0
    assert worst["orth"] <= ORTH


@pytest.mark.parametrize("k,n", [(5, 67), (17, 259), (64, 128)])
def test_a_pair_is_bitwise_the_same_alone_in_a_stack_and_broadcast(k, n):
    stacks = _stacks(k, n)
    a0, b0 = stacks[3][1][0], stacks[3][2][0]                        # the pair under test
    a1, b1 = stacks[1][1][1], stacks[1][2][1]                        # a filler
    a_stack, b_stack = np.stack([a0, a1, a0]), np.stack([b0, b1, b0])
    b_other = np.stack([b1, b0, b1])

    def runs(x, y, **kw):
        """every output of the four calls on (x, y), as one list"""
        pa, pb, th0 = _call("principal_vectors", x, y, **kw)
        p, h, th1 = _call("grassmann_log", x, y, **kw)
        yy, th2 = _call("grassmann_geodesic", x, y, TS, **kw)
        hs = h if h.ndim == 3 else h[None]
        ps = p if p.ndim == 3 else p[None]
        ye, sg = _call("grassmann_exp", ps, hs, [0.5, 1.0], **kw)
        return [pa, pb, th0, p, h, th1, yy, th2, ye, sg]

    alone = runs(a0, b0)
    again = runs(a0, b0)
    stack = runs(a_stack, b_stack)
    bcast = runs(a0, b_other)                                        # A broadcast: the pair sits at position 1
    for i, (x, y, s, c) in enumerate(zip(alone, again, stack, bcast)):
        assert not np.isnan(x).any(), i
        assert x.tobytes() == y.tobytes(), f"output {i}: two runs differ"
        assert x[0].tobytes() == s[0].tobytes() and x[0].tobytes() == s[2].tobytes(), f"output {i}: alone vs in a stack"
        assert x[0].tobytes() == c[1].tobytes(), f"output {i}: alone vs broadcast"


def test_cut_locus_is_refused_for_that_pair_only():
    k, n = 2, 8
    e = np.eye(n, dtype=np.float32)
    a = np.stack([e[:2], e[:2], e[:2]])
    b = np.stack([np.stack([e[0], e[2]]), np.stack([np.float32(np.cos(0.3)) * e[0] + np.float32(np.sin(0.3)) * e[2], e[1]]), np.stack([e[4], e[5]])])
    for name, extra in [("principal_vectors", ()), ("grassmann_log", ()), ("grassmann_geodesic", (TS,))]:
        with pytest.raises(ValueError, match=r"cut locus.*pi/2 - 1e-6.*indices \[0, 2\]"):
            _call(name, a, b, *extra)
        out = _call(name, a, b, *extra, check=False)
        for o in out:
            assert np.isnan(o[0]).all() and np.isnan(o[2]).all() and not np.isnan(o[1]).any(), name
    theta = _call("principal_vectors", a, b, check=False)[2]
    assert np.abs(theta[1] - np.array([0.3, 0.0])).max() <= BAR


def test_degenerate_bases_are_named():
    k, n = 3, 40
    rng = np.random.default_rng(5)
    a = rng.standard_normal((3, k, n)).astype(np.float32)
    b = rng.standard_normal((3, k, n)).astype(np.float32)
    b = b + 3 * a                                                    # well inside the domain
    bad = b.copy()
    bad[1, 2] = 0.0
    from diffusion_pullback_amd.geometry import DEGENERATE
    import re
    for name, extra in [("principal_vectors", ()), ("grassmann_log", ()), ("grassmann_geodesic", (0.5,))]:
        with pytest.raises(ValueError, match=re.escape(DEGENERATE) + r": indices \[1\]"):
            _call(name, a, bad, *extra)
        out = _call(name, a, bad, *extra, check=False)
        for o in out:
            assert np.isnan(o[1]).all() and not np.isnan(o[0]).any() and not np.isnan(o[2]).any(), name
    with pytest.raises(ValueError, match=re.escape(DEGENERATE) + r": indices \[1\]"):
        _call("grassmann_exp", bad, a, 0.5)
    y, sigma = _call("grassmann_exp", bad, a, 0.5, check=False)
    assert np.isnan(y[1]).all() and np.isnan(sigma[1]).all() and not np.isnan(y[0]).any() and not np.isnan(y[2]).any()
    y, sigma = _call("grassmann_exp", a, np.zeros_like(a), [0.0, 2.0])     # a zero tangent is no error: the geodesic stays where it is
    assert np.abs(sigma).max() == 0.0
    for d in range(3):
        assert R.max_angle(y[d, 1], a[d]) <= BAR


def test_rank_and_shape_limits():
    from diffusion_pullback_amd import geometry, lib
    so = lib.load()
    assert so.dpb_grassmann_scratch_bytes(2, 6, 65, 128) == 0 and so.dpb_grassmann_scratch_bytes(2, 6, 8, 7) == 0
    assert so.dpb_grassmann_scratch_bytes(2, 6, 64, 128) > 0
    x = torch.zeros(2, 65, 128, device=DEV)
    for fn, extra in [(geometry.principal_vectors, ()), (geometry.grassmann_log, ()), (geometry.grassmann_geodesic, (0.5,)), (geometry.grassmann_exp, (0.5,))]:
        with pytest.raises(ValueError, match="k = 65 rows per basis exceeds the rank 64"):
            fn(x, x, *extra)
        with pytest.raises(ValueError, match="exceeds their length"):
            fn(x[:, :9, :8], x[:, :9, :8], *extra)
        with pytest.raises(ValueError, match="must be"):
            fn(x[:, :4], x[:1, :5], *extra)
    with pytest.raises(ValueError, match="1 .. 64 parameters"):
        geometry.grassmann_geodesic(x[:, :4], x[:, :4], [])
