"""PullbackUNet.pullback_geodesic / curve_energy (dpb_geodesic_chain) on the toy DDPM, ADM and SD nets of tests/test_gpu_inv_jac_chain.py (side 8):
consistency with the engine's own passes and the two kernels, and accuracy against the float64 chain of tests/_geodesic_ref.py on the oracle's CPU
nets, whose gradient is autograd's of the energy itself.

The accuracy bars are measured on the reference side only (_bars), by the rule of tests/test_gpu_inv_jac_chain.py: the oracle chain runs in float32 and
in float64 on the CPU; d_step is their worst one-iteration difference with every iteration started from the float64 chain's curve, d_chain their worst
free-running difference.  curves: absolute, normalised by eta max ||g_i|| (the largest step of the chain); seg_h and stats (||J^T c||^2, ||g||^2,
||dP||^2): relative.  The device must stay within 8 d: it differs from the CPU float32 run in summation order only, a wrong gradient is an O(1) error.
m = 3 interior points, 3 iterations of the step-rule eta (taken from the float64 probe, rounded to fp32), lam = 0, slerp start between two samples.
Measured d (curves / seg_h / stats) and the device's worst ratio to it on an MI355X (the test prints both sets at every run -- they move by a factor of
two or so with the CPU's own float32 summation order):
  net, tap       d_step                        d_chain                       device / d, worst
  ddpm mid 0     5.4e-07  1.6e-06  4.1e-06     8.1e-07  1.1e-06  4.8e-06     1.3
  ddpm down 1    7.6e-07  2.5e-06  4.9e-06     1.6e-06  1.6e-06  8.9e-06     1.2
  ddpm up 1      6.0e-07  1.5e-06  3.9e-06     7.5e-07  2.7e-06  7.3e-06     1.7
  adm mid 0      1.4e-07  5.2e-07  7.6e-07     1.2e-06  3.8e-06  7.5e-06     1.8
  sd mid 0       3.3e-07  7.4e-07  1.8e-06     9.6e-07  1.8e-06  3.4e-06     1.8
  sd down 0      2.9e-07  6.7e-07  5.7e-07     5.9e-07  8.4e-07  1.6e-06     3.0
  sd up 1        3.6e-07  7.6e-07  1.5e-06     5.1e-07  7.6e-07  1.8e-06     2.6
At one eta a Jacobi chain need not go on descending (the float64 chain rises at iteration 2 on ddpm down 1, ddpm up 1 and adm mid); the device rises
where it does.  The driver (m = 4, max_iter 12, ddpm mid and sd mid): three accepted blocks, 12 iterations, as the float64 reference, whose decisions
have relative margins >= 0.048; energies 7.6e-07 (ddpm; the float32 oracle driver: 1.6e-06) and 1.4e-05 (sd; 8.1e-06) from the float64 ones."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _geodesic_ref as R
import test_gpu_inv_jac_chain as IJ

pytestmark = pytest.mark.gpu

F32, BF, F16 = torch.float32, torch.bfloat16, torch.float16
T, M, ITERS = 301.0, 3, 3
KEYS = ("curves", "seg_h", "stats")


def _dev():
    return IJ._dev()


@functools.lru_cache(maxsize=None)
def _curve(kind, m):
    """(P [m + 2, C, H, W] fp32: the slerp start between two samples of the toy set, ctx [m + 2, L, D] or None: a row per point)"""
    from diffusion_pullback_amd.pullback import geodesic_init
    _, _, x, ctx = IJ._model(kind)
    c = None if ctx is None else torch.cat([ctx, ctx + 0.1, ctx - 0.1])[:m + 2]
    return geodesic_init(x[0], x[1], m, "slerp"), c


def _net(kind, dtype=F32, m=M):
    return IJ._net(kind, dtype, max_batch=m + 2, max_rank=m)


def _chain(net, tap, P, ctx, eta, lam, iters, final=True):
    """the engine call, on the host as a dict of the reference's keys"""
    curves, seg_h, seg_x, stats, csq = net.engine.geodesic_chain(P.to(_dev()), T, None if ctx is None else ctx.to(_dev()), tap, eta, lam, iters, final)
    return {"curves": curves.cpu(), "seg_h": seg_h.cpu(), "seg_x": seg_x.cpu(), "stats": stats.cpu(), "csq": csq.cpu()}


def _eta(net, tap, P, ctx, lam=0.0):
    r = _chain(net, tap, P, ctx, 0.0, lam, 1, False)
    return float(np.float32(R.step_rule(r)))


@pytest.mark.parametrize("dtype", [F32, BF, F16])
@pytest.mark.parametrize("kind", ["ddpm", "adm", "sd"])
def test_chain_is_its_step_by_step_composition(kind, dtype):
    """a 3-iteration chain is torch.equal to eng.forward (the end points, once) and per iteration eng.primal / eng.read / dpb_geodesic_cotangents /
    eng.vjp / dpb_geodesic_update; the last row is one more forward pass; the probe (eta = 0) moves nothing"""
    from diffusion_pullback_amd.engine import geodesic_cotangents, geodesic_update
    tap, lam = ("mid", 0), 0.3
    P, ctx = _curve(kind, M)
    net = _net(kind, dtype)
    eng = net.engine
    eta = _eta(net, tap, P, ctx, lam)
    assert np.isfinite(eta) and eta > 0
    r = _chain(net, tap, P, ctx, eta, lam, ITERS)
    assert torch.equal(r["curves"][0], P) and all(torch.isfinite(r[k]).all() for k in r) and (r["stats"][..., 3] == 0).all()
    probe = _chain(net, tap, P, ctx, 0.0, lam, 1, False)
    assert torch.equal(probe["curves"][1], P) and torch.equal(probe["seg_h"][0], r["seg_h"][0]) and torch.equal(probe["csq"][0], r["csq"][0])
    assert torch.isnan(probe["seg_h"][1]).all() and torch.isnan(probe["seg_x"][1]).all() and (probe["stats"][0, :, 2] == 0).all()
    d = _dev()
    cd = None if ctx is None else ctx.to(d)
    ends = lambda a: None if a is None else torch.stack([a[0], a[-1]])
    he = eng.forward(ends(P.to(d)), T, ends(cd), tap).flatten(1)
    cur = P.to(d)
    for j in range(ITERS + 1):
        if j < ITERS:
            eng.primal(cur[1:-1], T, None if cd is None else cd[1:-1], tap)
            hi = eng.read(tap).flatten(1)
        else:
            hi = eng.forward(cur[1:-1], T, None if cd is None else cd[1:-1], tap).flatten(1)
        cot, seg, csq = geodesic_cotangents(torch.cat([he[:1], hi, he[1:]]).contiguous())
        assert torch.equal(seg.cpu(), r["seg_h"][j]), (j, "seg_h")
        if j == ITERS:
            assert torch.equal(geodesic_cotangents(cur.flatten(1))[1].cpu(), r["seg_x"][j])
            break
        W = eng.vjp(tap, cot)
        nxt, stats, xseg = geodesic_update(cur.flatten(1).contiguous(), W, eta, lam)
        assert torch.equal(csq.cpu(), r["csq"][j]) and torch.equal(stats.cpu(), r["stats"][j]) and torch.equal(xseg.cpu(), r["seg_x"][j]), j
        assert torch.equal(nxt.view_as(cur).cpu(), r["curves"][j + 1]), j
        cur = nxt.view_as(cur)
    if dtype == F32:                                                             # the first step of the step rule's eta descends (a Jacobi chain at
        E = 0.5 * r["seg_h"].sum(1) + 0.5 * lam * r["seg_x"].sum(1)               # one eta need not go on descending: the driver's halving is for that)
        assert E[1] < E[0], E


@pytest.mark.parametrize("kind", ["ddpm", "sd"])
def test_block_additivity_and_final_energy(kind):
    """one call of 4 iterations is bitwise two calls of 2; final_energy=False leaves NaN in the last row, changes nothing else and runs one forward pass
    fewer by the engine's launch counter"""
    tap = ("mid", 0)
    P, ctx = _curve(kind, M)
    net = _net(kind)
    eta = _eta(net, tap, P, ctx)
    full = _chain(net, tap, P, ctx, eta, 0.0, 4)
    n_full = net.engine.stats()[0]
    a = _chain(net, tap, P, ctx, eta, 0.0, 2)
    b = _chain(net, tap, a["curves"][2], ctx, eta, 0.0, 2)
    assert torch.equal(full["curves"], torch.cat([a["curves"], b["curves"][1:]]))
    for k in ("seg_h", "seg_x"):
        assert torch.equal(full[k][:3], a[k]) and torch.equal(full[k][2:], b[k]), k
    for k in ("stats", "csq"):
        assert torch.equal(full[k], torch.cat([a[k], b[k]])), k
    nf = _chain(net, tap, P, ctx, eta, 0.0, 4, False)
    n_nf = net.engine.stats()[0]
    assert torch.isnan(nf["seg_h"][4]).all() and torch.isnan(nf["seg_x"][4]).all()
    assert all(torch.equal(nf[k], full[k]) for k in ("curves", "stats", "csq")) and torch.equal(nf["seg_h"][:4], full["seg_h"][:4])
    assert torch.equal(nf["seg_x"][:4], full["seg_x"][:4])
    _chain(net, tap, P, ctx, eta, 0.0, 3, False)
    n3 = net.engine.stats()[0]
    _chain(net, tap, P, ctx, eta, 0.0, 3, True)
    n3f = net.engine.stats()[0]
    one_pass, one_iter = n_full - n_nf, n_nf - n3
    print(f"{kind}: launches 4 iterations {n_nf}, + final pass {one_pass}, one iteration {one_iter}")
    assert one_pass > 0 and n3f - n3 == one_pass and one_iter > 2 * one_pass - 8      # an iteration: a primal and an adjoint pass
    with pytest.raises(Exception):                                                 # the call leaves no primal state, as dpb_forward
        net.engine.vjp(tap, torch.zeros(M, net.engine.tap_numel(tap)))


def _dist(a, b, key, unit):
    """how far two runs are apart in one quantity: the curves absolute over the largest step, the sums relative"""
    x, y = a[key].double(), b[key].double()
    if key == "stats":
        x, y = x[..., :3], y[..., :3]
    d = (x - y).abs()
    return float(d.max()) / unit if key == "curves" else float((d / y.abs()).max())


def _resync(run_one, ref64):
    """one-iteration runs started from the float64 chain's curves: the curve reached, both energy rows and the statistics of every iteration"""
    out = {k: [] for k in KEYS}
    for j in range(ITERS):
        r = run_one(ref64["curves"][j].float())
        out["curves"].append(r["curves"][1].double()); out["seg_h"].append(r["seg_h"].double()); out["stats"].append(r["stats"][0].double())
    return {k: torch.stack(v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _bars(kind, tap):
    """(eta, unit, ref64, resync64, d_step, d_chain) of the float64 and float32 oracle chains"""
    P, ctx = _curve(kind, M)
    g64, g32 = R.get_hs(kind, tap, torch.float64, T, ctx), R.get_hs(kind, tap, torch.float32, T, ctx)
    eta = float(np.float32(R.step_rule(R.geodesic_ref(g64, P, 0.0, 0.0, 1, torch.float64, False))))
    ref64, ref32 = R.geodesic_ref(g64, P, eta, 0.0, ITERS, torch.float64), R.geodesic_ref(g32, P, eta, 0.0, ITERS, torch.float32)
    unit = eta * float(ref64["stats"][..., 1].max().sqrt())
    one = lambda g, dt: (lambda c: R.geodesic_ref(g, c, eta, 0.0, 1, dt))
    rs64, rs32 = _resync(one(g64, torch.float64), ref64), _resync(one(g32, torch.float32), ref64)
    return eta, unit, ref64, rs64, {k: _dist(rs32, rs64, k, unit) for k in KEYS}, {k: _dist(ref32, ref64, k, unit) for k in KEYS}


CASES = [("ddpm", ("mid", 0)), ("ddpm", ("down", 1)), ("ddpm", ("up", 1)), ("adm", ("mid", 0)), ("sd", ("mid", 0)), ("sd", ("down", 0)), ("sd", ("up", 1))]


@pytest.mark.parametrize("kind,tap", CASES)
def test_accuracy_against_the_float64_chain(kind, tap):
    """free-running within 8 d_chain, re-synchronised within 8 d_step; the device's step rule agrees with the float64 one"""
    P, ctx = _curve(kind, M)
    eta, unit, ref64, rs64, d_step, d_chain = _bars(kind, tap)
    net = _net(kind)
    free = _chain(net, tap, P, ctx, eta, 0.0, ITERS)
    rs = _resync(lambda c: _chain(net, tap, c, ctx, eta, 0.0, 1), ref64)
    print(f"{kind} {tap}: eta {eta:.4e} unit {unit:.3e} d_step " + " ".join(f"{k} {d_step[k]:.3e}" for k in KEYS) + " | d_chain "
          + " ".join(f"{k} {d_chain[k]:.3e}" for k in KEYS))
    got_step, got_chain = {k: _dist(rs, rs64, k, unit) for k in KEYS}, {k: _dist(free, ref64, k, unit) for k in KEYS}
    print("   device:  step " + " ".join(f"{k} {got_step[k]:.3e}" for k in KEYS) + " | chain " + " ".join(f"{k} {got_chain[k]:.3e}" for k in KEYS)
          + f" | worst ratio {max(max(got_step[k] / d_step[k], got_chain[k] / d_chain[k]) for k in KEYS):.2f}")
    for k in KEYS:
        assert got_step[k] <= 8 * d_step[k], (k, got_step[k], d_step[k])
        assert got_chain[k] <= 8 * d_chain[k], (k, got_chain[k], d_chain[k])
    assert abs(_eta(net, tap, P, ctx) - eta) <= 1e-4 * eta
    E = 0.5 * free["seg_h"].sum(1)
    assert E[1] < E[0] and ((E[1:] < E[:-1]) == (ref64["seg_h"].sum(1)[1:] < ref64["seg_h"].sum(1)[:-1])).all()   # rises where the float64 chain rises


@functools.lru_cache(maxsize=None)
def _driver_ref(kind, dtype):
    P, ctx = _curve(kind, 4)
    g = R.get_hs(kind, ("mid", 0), dtype, T, ctx)
    return R.descent_ref(g, P, 0.0, None, max_iter=12, tol=1e-4, check_every=4, dtype=dtype)


@pytest.mark.parametrize("kind", ["ddpm", "sd"])
def test_driver_takes_the_decisions_of_the_float64_reference(kind):
    """pullback_geodesic (fp32 engine, m = 4, max_iter 12) against the float64 driver of tests/_geodesic_ref.py: the same accept / reject sequence and
    iterations -- claimed because every decision of the reference has a relative margin >= 1e-3, asserted here on the CPU; the energies within 8 times
    the float32 oracle driver's distance from the float64 one; curve_energy of the result is the chain's last row bit for bit"""
    tap = ("mid", 0)
    P, ctx = _curve(kind, 4)
    _, ref = _driver_ref(kind, torch.float64)
    _, ref32 = _driver_ref(kind, torch.float32)
    assert min(ref["margins"]) >= 1e-3, ref["margins"]
    assert ref32["decisions"] == ref["decisions"]
    bar = max(abs(a - b) / b for a, b in zip(ref32["energy"], ref["energy"]))
    net = _net(kind, m=4)
    d = _dev()
    cd = None if ctx is None else ctx.to(d)
    curve, info = net.pullback_geodesic(P[:1].to(d), P[-1:].to(d), T, n_points=4, op=tap[0], block_idx=tap[1], encoder_hidden_states=cd, init="slerp",
                                        max_iter=12, tol=1e-4, check_every=4)
    got = max(abs(a - b) / b for a, b in zip(info["energy"], ref["energy"]))
    print(f"{kind}: decisions {info['decisions']} iterations {info['iterations']} rises {info['rises']} / {ref['rises']} energy {info['energy']} | float64 {ref['energy']} | bar {bar:.3e} device {got:.3e}")
    assert info["decisions"] == ref["decisions"] and info["iterations"] == ref["iterations"] and info["halvings"] == ref["halvings"]
    assert info["converged"] == ref["converged"] and len(info["energy"]) == len(ref["energy"])
    assert got <= 8 * bar, (got, bar)
    assert info["monotone"] and info["energy"][-1] < info["start"]["energy"] and info["energy"][0] == info["start"]["energy"]
    assert abs(info["step_size"] - ref["step_size"]) <= 1e-4 * ref["step_size"] and info["grad_norm"].shape == (4,)
    assert curve.shape == P.shape and torch.equal(curve[0].cpu(), P[0]) and torch.equal(curve[-1].cpu(), P[-1])
    ruler = net.curve_energy(curve, T, op=tap[0], block_idx=tap[1], encoder_hidden_states=cd)
    assert torch.equal(ruler["seg_h"], info["seg_h"]) and torch.equal(ruler["seg_x"], info["seg_x"])
    assert ruler["energy"] == info["energy"][-1] == info["energy_h"] and ruler["length_h"] == info["length_h"] and ruler["uniformity"] == info["uniformity"]
    start = net.curve_energy(P.to(d), T, op=tap[0], block_idx=tap[1], encoder_hidden_states=cd)
    assert start["energy"] == info["start"]["energy"] and start["uniformity"] == info["start"]["uniformity"]
    lin = net.pullback_geodesic(P[:1].to(d), P[-1:].to(d), T, n_points=4, op=tap[0], block_idx=tap[1], encoder_hidden_states=None if cd is None else cd[:1],
                                init="linear", step_size=info["step_size"], max_iter=4)[1]       # the other start, one context row for the curve
    assert lin["attempted"] == 4 and lin["energy"][-1] <= lin["energy"][0] and lin["start"]["energy"] != info["start"]["energy"]


def test_refusals_and_non_finite_points():
    from diffusion_pullback_amd import lib as L
    kind, tap = "ddpm", ("mid", 0)
    P, _ = _curve(kind, 4)
    net = _net(kind, m=4)
    d = _dev()
    kw = dict(t=T, op=tap[0], block_idx=tap[1])
    with pytest.raises(ValueError, match="max_batch=6"):
        net.pullback_geodesic(P[:1], P[-1:], n_points=5, **kw)
    with pytest.raises(ValueError, match="max_batch=6"):
        net.curve_energy(torch.cat([P, P[:1]]), **kw)
    with pytest.raises(ValueError, match="lam=-0.5"):
        net.pullback_geodesic(P[:1], P[-1:], n_points=4, lam=-0.5, **kw)
    clean = _chain(net, tap, P, None, 1e-3, 0.0, 1)
    bad = P.clone()
    bad[2, 1, 3, 3] = float("nan")
    with pytest.raises(ValueError, match="point 2 .* iteration 0"):
        net.pullback_geodesic(P[:1], P[-1:], n_points=4, init=bad, step_size=1e-3, max_iter=4, **kw)
    curve, info = net.pullback_geodesic(P[:1], P[-1:], n_points=4, init=bad, step_size=1e-3, max_iter=4, check=False, **kw)
    # the point's own row and its two neighbours', whose cotangents read its activation; every other row is the clean step's, bit for bit
    assert torch.isnan(curve[1:4]).all() and torch.equal(curve[[0, 4, 5]], clean["curves"][1][[0, 4, 5]])
    assert info["converged"] is False and info["iterations"] == 0
    # straight at the C entry point
    eng, lib, m = net.engine, L.load(), 4
    buf = eng.tape.taps[tap]
    need = int(lib.dpb_geodesic_chain_scratch_bytes(eng.h, buf, m))
    assert need > 0 and lib.dpb_geodesic_chain_scratch_bytes(eng.h, -1, m) == 0 and lib.dpb_geodesic_chain_scratch_bytes(eng.h, buf, 0) == 0
    sc = torch.empty(need + 512, dtype=torch.uint8, device=d)
    base = sc.data_ptr() + (-sc.data_ptr()) % 256
    Pd = P.to(d)
    curves = torch.full((2, m + 2, *P.shape[1:]), 7.0, device=d)
    f64 = lambda *s: torch.full(s, 7.0, dtype=torch.float64, device=d)
    sh, sx, st, cq = f64(2, m + 1), f64(2, m + 1), f64(1, m, 4), f64(1, m)

    def call(tap_buf=buf, m_=m, t=T, eta=1e-3, lam=0.0, iters=1, scratch=base, nbytes=need):
        return lib.dpb_geodesic_chain(eng.h, tap_buf, Pd.data_ptr(), m_, t, None, eta, lam, iters, 1, curves.data_ptr(), sh.data_ptr(), sx.data_ptr(),
                                      st.data_ptr(), cq.data_ptr(), C.c_void_p(scratch), nbytes)
    for k, word in ((dict(tap_buf=eng.tape.temb_in), b"tap buffer"), (dict(tap_buf=10 ** 6), b"tap buffer"), (dict(m_=0), b"m=0"), (dict(m_=5), b"m=5"),
                    (dict(iters=0), b"iters=0"), (dict(t=float("nan")), b"finite"), (dict(eta=float("inf")), b"finite"), (dict(lam=-1.0), b"lambda"),
                    (dict(nbytes=need - 1), b"scratch of"), (dict(scratch=base + 8), b"aligned")):
        assert call(**k) != 0 and word in lib.dpb_last_error(), (k, lib.dpb_last_error())
    torch.cuda.synchronize()
    assert (curves == 7.0).all() and (sh == 7.0).all() and (st == 7.0).all()       # a refused call has touched nothing
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(curves.cpu(), clean["curves"]) and torch.equal(sh.cpu(), clean["seg_h"]) and torch.equal(st.cpu(), clean["stats"])
    small = IJ._net(kind, max_batch=1, max_rank=3)                                 # the two end points need a batch of 2
    with pytest.raises(ValueError, match="max_batch=1"):
        small.pullback_geodesic(P[:1], P[-1:], n_points=1, **kw)
    with pytest.raises(L.DpbError, match="max_batch=1"):
        small.engine.geodesic_chain(P[:3].to(d), T, None, tap, 1e-3, 0.0, 1)
