"""PullbackUNet.newton_h_chain (dpb_newton_h_chain) on the toy DDPM, ADM and SD nets of tests/test_gpu_inv_jac_chain.py (side 8, per-sample timesteps,
three chains): bitwise its step-by-step composition from the engine's passes and the entry points of csrc/cgls.hip, accurate against the float64
chain of tests/_cgls_ref.py on the oracle's CPU nets, and of the sign the documentation states.

Accuracy (fp32 engine; 2 outer steps of 8 inner iterations, tol = 0, mu = 0.1 sigma_1^2, each chain towards a shift of a quarter of ||h0|| along a
Gaussian direction, seed 34, both signs): the device within 8 d of the float64 chain in states, h_shift and h_dist, d the float32 oracle's own
distance from it, absolute over the shift asked for -- measured on the reference side only (tests/_cgls_cases.py).  Measured d on the machine that ran the device (the test prints them, and the device's distances beside them, at every run):
  net, tap       states    h_shift   h_dist     device / d
  ddpm mid 0     8.9e-08   8.3e-07   1.8e-06    1.06  0.45  0.50
  ddpm up 1      3.2e-08   1.4e-07   8.0e-07    0.95  0.90  1.07
  adm mid 0      2.8e-08   5.3e-08   1.7e-07    1.33  1.18  1.08
  sd mid 0       4.2e-09   1.9e-07   2.8e-07    1.02  1.65  2.25
  sd down 0      8.9e-09   1.7e-07   3.4e-07    2.24  2.12  1.85
16-bit engines are held to the bitwise composition and to finiteness only.  The composition test runs at a fiftieth of that shift: the search direction
goes into the tangent pass unnormalised, and at the full shift the fp16 engine of the toy SD net (gain ~ 280) overflows in the second outer step, which
the solver reports as flag 3 with NaN in that chain alone."""
import numpy as np
import pytest
import torch

import _cgls_cases as K
from test_gpu_inv_jac_chain import DIRS, SIGNS, TS, _dev, _model, _net

pytestmark = pytest.mark.gpu

F32, BF, F16 = torch.float32, torch.bfloat16, torch.float16
MID = [("ddpm", ("mid", 0)), ("adm", ("mid", 0)), ("sd", ("mid", 0))]


def _ctx(kind):
    ctx = _model(kind)[3]
    return None if ctx is None else ctx.to(_dev())


def _compose(eng, tap, x, ts, ctx, U, dirs, signs, scale, steps, iters, mu_abs, mu_rel, tol, radius):
    """the chain, one entry point at a time"""
    from diffusion_pullback_amd import engine as E
    states, hist, stats, shift = [x], [], [], []
    h0 = None
    for j in range(steps + 1):
        eng.primal(states[-1], ts, ctx, tap)
        h = eng.read(tap).reshape(x.shape[0], -1)
        h0 = h if h0 is None else h0
        shift.append(E.shift_stats(h, h0, U, dirs, signs))
        if j == steps:
            break
        res = E.newton_residual(h0, h, U, dirs, signs, scale, (j + 1) / steps)
        S, hi = E.cgls_init(res, eng.vjp(tap, res), mu_abs, mu_rel, tol)
        hs = [hi]
        for _ in range(iters):
            E.cgls_h_step(S, eng.jvp(tap, S.p))
            hs.append(E.cgls_x_step(S, eng.vjp(tap, S.r), tol))
        out, st = E.newton_update(states[-1].reshape(x.shape[0], -1), S.delta, S.state, radius)
        states.append(out.reshape(x.shape)); hist.append(torch.stack(hs)); stats.append(st)
    return torch.stack(states), torch.stack(hist), torch.stack(stats), torch.stack(shift)


@pytest.mark.parametrize("dtype", [F32, BF, F16])
@pytest.mark.parametrize("kind,tap", MID)
def test_the_chain_is_bitwise_its_composition(kind, tap, dtype):
    """without and with a clamp that bites; final_shift=False leaves NaN in the last shift and changes nothing else"""
    _, _, x, _ = _model(kind)
    net = _net(kind, dtype)
    eng = net.engine
    u, scale, _ = K.chain_inputs(kind, tap)
    # a fiftieth of the accuracy test's shift: the search direction p = J^T res goes into the tangent pass as it is, and at the full shift its fp16
    # activations on the toy SD net (gain sigma_1 ~ 280) pass 65504 in the second outer step -- the solver then flags the row (3) and both routes hold
    # the same NaNs, which says nothing about the composition
    scale = [s / 50 for s in scale]
    U = u.T.contiguous().to(_dev())
    xd = x.to(_dev())
    free = eng.newton_h_chain(xd, TS, _ctx(kind), tap, U, DIRS, SIGNS, scale, 2, 2, 0.5, 0.1, 1e-5, 0.0)
    clamp = 0.25 * float(free[2][..., 1].min().sqrt())                                         # a quarter of the shortest unclamped step
    for radius in (0.0, clamp):
        args = (U, DIRS, SIGNS, scale, 2, 2, 0.5, 0.1, 1e-5, radius)
        got = eng.newton_h_chain(xd, TS, _ctx(kind), tap, *args)
        want = _compose(eng, tap, xd, TS, _ctx(kind), *args)
        for a, b, name in zip(got, want, ("states", "hist", "step_stats", "shift")):
            assert torch.equal(a, b), (kind, dtype, radius, name)
        assert all(torch.isfinite(a).all() for a in got) and torch.equal(got[0][0], xd)
        clip = got[2][..., 2]
        assert (clip == 1).all() if radius == 0 else ((clip < 1).all() and (clip > 0).all())
        if radius:                                                                             # a clamped step has the radius for its length
            step = (got[0][1:] - got[0][:-1]).reshape(2, 3, -1).double().norm(dim=2)
            # (to the fp32 rounding of the states: sqrt(N) half-ulps of the largest |x|, twice for the difference)
            assert torch.allclose(step, torch.full_like(step, radius), rtol=1e-6, atol=x[0].numel() ** 0.5 * 2.0 ** -23 * float(xd.abs().max()))
    nf = eng.newton_h_chain(xd, TS, _ctx(kind), tap, *args, final_shift=False)
    assert torch.isnan(nf[3][-1]).all() and torch.equal(nf[3][:-1], got[3][:-1]) and all(torch.equal(a, b) for a, b in zip(nf[:3], got[:3]))


@pytest.mark.parametrize("kind,tap", K.CASES)
def test_accuracy_against_the_float64_chain(kind, tap):
    _, _, x, _ = _model(kind)
    ref64, d, sigma = K.chain_bars(kind, tap)
    u, scale, mu = K.chain_inputs(kind, tap)
    net = _net(kind)
    r = net.newton_h_chain(x=x.to(_dev()), t=TS, u=u, dirs=DIRS, signs=SIGNS, scale=scale, steps=K.CHAIN["steps"], iters=K.CHAIN["iters"], damping=0.0,
                           mu=mu, tol=K.CHAIN["tol"], encoder_hidden_states=_ctx(kind), op=tap[0], block_idx=tap[1])
    got = K.chain_dist({"states": r["states"].reshape(3, K.CHAIN["steps"] + 1, -1).cpu().numpy(), "h_shift": r["h_shift"].cpu().numpy(),
                        "h_dist": r["h_dist"].cpu().numpy()}, ref64, sigma)
    print(f"{kind} {tap}: float32 oracle " + " ".join(f"{k} {d[k]:.3e}" for k in K.KEYS) + " | device " + " ".join(f"{k} {got[k]:.3e}" for k in K.KEYS)
          + " | device / d " + " ".join(f"{got[k] / d[k]:.2f}" for k in K.KEYS))
    for k in K.KEYS:
        assert got[k] <= 8 * d[k], (k, got[k], d[k])
    assert (r["h_shift"][:, 1:] > 0).all() and (r["inner_iterations"] == K.CHAIN["iters"]).all() and (r["clip"] == 1).all()
    assert np.allclose(r["delta_norm"].cpu().numpy(), ref64["delta_norm"], rtol=1e-4)
    off2 = torch.clamp(r["h_dist"] ** 2 - r["h_shift"] ** 2, min=0)                             # h_off^2 = h_dist^2 - h_shift^2, to fp64 rounding of the squares
    assert torch.allclose(r["h_off"] ** 2, off2, rtol=0, atol=1e-12 * float((r["h_dist"] ** 2).max()))
    assert r["gamma"].shape == (3, K.CHAIN["steps"], K.CHAIN["iters"] + 1)


@pytest.mark.parametrize("kind,tap", MID)
def test_a_chain_with_sign_plus_one_moves_h_along_its_direction(kind, tap):
    """the opposite of inv_jac_chain, which keeps the reference's sign"""
    _, _, x, _ = _model(kind)
    net = _net(kind)
    u, scale, _ = K.chain_inputs(kind, tap)
    kw = dict(x=x.to(_dev()), t=TS, u=u, dirs=DIRS, encoder_hidden_states=_ctx(kind), op=tap[0], block_idx=tap[1])
    r = net.newton_h_chain(signs=[1.0] * 3, scale=scale, steps=2, iters=4, **kw)
    old = net.inv_jac_chain(signs=[1.0] * 3, steps=2, step_size=0.5, **kw)
    assert (r["h_shift"][:, 1:] > 0).all() and (old["h_shift"][:, 1:] < 0).all()
    assert (r["h_shift"][:, 2] > r["h_shift"][:, 1]).all()                                     # further at every outer step
    neg = net.newton_h_chain(signs=[-1.0] * 3, scale=scale, steps=2, iters=4, **kw)              # a negative sign IS the negative direction
    flip = net.newton_h_chain(signs=[1.0] * 3, scale=[-s for s in scale], steps=2, iters=4, **kw)
    assert (neg["h_shift"][:, 1:] > 0).all() and (flip["h_shift"][:, 1:] < 0).all()


def test_groups_and_one_chain_alone():
    """five chains on an engine of max_batch 3 run as groups of 3 and 2, bitwise the two calls; steps = 2 is bitwise two calls of steps = 1 only when
    the target of the second is restated, so that is not claimed: the chain keeps h0 from its own step 0"""
    kind, tap = "ddpm", ("mid", 0)
    _, _, x, _ = _model(kind)
    net = _net(kind)
    u, scale, _ = K.chain_inputs(kind, tap)
    x5 = torch.cat([x, x[:2] + 0.1]).to(_dev())
    t5, d5, s5, sc5 = TS + [TS[0], TS[2]], DIRS + [1, 0], SIGNS + [-1.0, 1.0], scale + [scale[0], 2 * scale[1]]
    kw = dict(u=u, steps=2, iters=3, op=tap[0], block_idx=tap[1], radius=0.5)
    r = net.newton_h_chain(x=x5, t=t5, dirs=d5, signs=s5, scale=sc5, **kw)
    a = net.newton_h_chain(x=x5[:3], t=t5[:3], dirs=d5[:3], signs=s5[:3], scale=sc5[:3], **kw)
    b = net.newton_h_chain(x=x5[3:], t=t5[3:], dirs=d5[3:], signs=s5[3:], scale=sc5[3:], **kw)
    assert r["states"].shape == (5, 3, *x.shape[1:]) and r["gamma"].shape == (5, 2, 4) and r["inner_iterations"].shape == (5, 2)
    assert all(torch.equal(r[k], torch.cat([a[k], b[k]])) for k in r)


def test_error_paths_leave_a_message_and_the_next_call_is_unaffected():
    from diffusion_pullback_amd import lib as L
    kind, tap = "ddpm", ("mid", 0)
    _, _, x, _ = _model(kind)
    net = _net(kind)
    eng = net.engine
    u, scale, _ = K.chain_inputs(kind, tap)
    U, xd = u.T.contiguous().to(_dev()), x.to(_dev())
    ref = eng.newton_h_chain(xd, TS, None, tap, U, DIRS, SIGNS, scale, 2, 2)

    def refused(word, xs=xd, t=TS, dirs=DIRS, signs=SIGNS, sc=scale, steps=2, iters=2, **kw):
        with pytest.raises(L.DpbError) as e:
            eng.newton_h_chain(xs, t, None, tap, U, dirs, signs, sc, steps, iters, **kw)
        assert word in str(e.value) and word.encode() in L.load().dpb_last_error(), (word, str(e.value))

    refused("steps=0", steps=0)
    refused("iters=-1", iters=-1)
    refused("dir[1]=2", dirs=[0, 2, 1])
    refused("sign[2]", signs=[1.0, 1.0, float("inf")])
    refused("scale[0]", sc=[float("nan")] + scale[1:])
    refused("t[1]", t=[1.0, float("nan"), 2.0])
    refused("radius", radius=-1.0)
    refused("mu_rel", mu_rel=-0.1)
    refused("tol", tol=float("nan"))
    refused("n=4", xs=torch.cat([xd, xd[:1]]), t=TS + [1.0], dirs=DIRS + [0], signs=SIGNS + [1.0], sc=scale + [1.0])
    lib, buf = L.load(), eng.tape.taps[tap]
    assert lib.dpb_newton_h_chain_scratch_bytes(eng.h, buf, 3) > 0 and lib.dpb_newton_h_chain_scratch_bytes(eng.h, -1, 3) == 0
    with pytest.raises(L.DpbError):                                  # the call leaves no primal state, as dpb_forward
        eng.vjp(tap, torch.zeros(3, eng.tap_numel(tap)))
    again = eng.newton_h_chain(xd, TS, None, tap, U, DIRS, SIGNS, scale, 2, 2)
    assert all(torch.equal(a, b) for a, b in zip(again, ref))
    # a direction that is not finite: NaN in exactly that chain, named by check=True
    bad = u.clone(); bad[3, 1] = float("nan")
    kw = dict(x=xd, t=TS, u=bad, dirs=[0, 1, 0], signs=SIGNS, scale=scale, steps=2, iters=2, op=tap[0], block_idx=tap[1])
    with pytest.raises(ValueError, match="chain 1 .* step 0"):
        net.newton_h_chain(**kw)
    r = net.newton_h_chain(check=False, **kw)
    assert torch.isnan(r["states"][1, 1:]).all() and torch.isfinite(r["states"][[0, 2]]).all() and r["flag"][1].tolist() == [3, 3]
