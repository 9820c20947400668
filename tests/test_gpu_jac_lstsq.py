"""PullbackUNet.jac_lstsq (dpb_jac_lstsq) on the toy DDPM, ADM and SD nets of tests/test_gpu_inv_jac_chain.py (side 8, per-sample timesteps, three
rows): bitwise the same steps composed from the engine's own passes and the solver's entry points, and accurate against the float64 restatement of
tests/_cgls_ref.py and the dense solve on the oracle's CPU nets.

Accuracy (fp32 engine; c Gaussian, seed 34; mu = 0.1 sigma_1^2 with sigma_1 the largest singular value of the dense float64 Jacobians of the three
samples), two regimes, the bars measured on the reference side only (tests/_cgls_cases.py):
  fixed      iters = 8, tol = 0: the device within 8 d of the float64 restatement, d the float32 oracle's own distance from it, relative in ||delta||;
  converged  iters = 32, tol = 1e-6: the float64 restatement within 4e-6 of the dense solve (asserted on the CPU), the device within 8 d of the dense
             solve, d the float32 oracle's distance from it, with `converged` set and at most 32 iterations.
Measured d on the machine that ran the device (the test prints them, and the device's distances beside them, at every run; d moves by a factor of
two or so with the CPU's own float32 summation order):
  net, tap       fixed d     device / d    converged d   device / d   float64 to dense   iterations float64, device
  ddpm mid 0     1.5e-06     2.26          1.8e-06       0.81         6.4e-07            12 .. 15, 13 .. 18
  ddpm up 1      1.4e-06     1.09          1.3e-06       1.24         8.7e-07            17 .. 19, 18 .. 22
  adm mid 0      5.5e-07     1.21          8.8e-07       1.10         9.0e-07            19 .. 20, 19 .. 21
  sd mid 0       1.8e-05     0.51          1.6e-06       1.12         8.2e-07            12 .. 15, 13 .. 18
  sd down 0      4.9e-05     0.97          1.1e-06       1.12         1.1e-06            12 .. 14, 13 .. 16
16-bit engines are held to the bitwise composition and to finiteness only: their tangent and adjoint passes are not exact transposes of each other,
and no accuracy is claimed."""
import ctypes as C

import numpy as np
import pytest
import torch

import _cgls_cases as K
from test_gpu_inv_jac_chain import TS, _dev, _model, _net

pytestmark = pytest.mark.gpu

F32, BF, F16 = torch.float32, torch.bfloat16, torch.float16
MID = [("ddpm", ("mid", 0)), ("adm", ("mid", 0)), ("sd", ("mid", 0))]


def _ctx(kind):
    ctx = _model(kind)[3]
    return None if ctx is None else ctx.to(_dev())


def _compose(eng, tap, c, mu_abs, mu_rel, tol, iters):
    """the steps of dpb_jac_lstsq from eng.vjp / eng.jvp and the solver's entry points"""
    from diffusion_pullback_amd import engine as E
    S, h = E.cgls_init(c, eng.vjp(tap, c), mu_abs, mu_rel, tol)
    hist = [h]
    for _ in range(iters):
        E.cgls_h_step(S, eng.jvp(tap, S.p))
        hist.append(E.cgls_x_step(S, eng.vjp(tap, S.r), tol))
    return S, torch.stack(hist)


@pytest.mark.parametrize("dtype", [F32, BF, F16])
@pytest.mark.parametrize("kind,tap", MID)
def test_the_call_is_bitwise_its_composition(kind, tap, dtype):
    """three samples at three timesteps, one right-hand side each; then one sample with three right-hand sides (the same call)"""
    _, _, x, _ = _model(kind)
    net = _net(kind, dtype)
    eng = net.engine
    c = K.rhs(kind, tap).to(_dev())
    for xs, ts, ctx in ((x, TS, _ctx(kind)), (x[:1], TS[0], None if _ctx(kind) is None else _ctx(kind)[:1])):
        eng.primal(xs.to(_dev()), ts, ctx, tap)
        delta, resid, hist = eng.jac_lstsq(tap, c, 0.5, 0.1, 1e-5, 3, return_resid=True)
        S, hc = _compose(eng, tap, c, 0.5, 0.1, 1e-5, 3)
        assert torch.equal(delta, S.delta) and torch.equal(resid, S.r) and torch.equal(hist, hc), (kind, dtype)
        assert torch.isfinite(delta).all() and torch.isfinite(hist).all() and (hist[..., 3] == 0).all()
        again = eng.jac_lstsq(tap, c, 0.5, 0.1, 1e-5, 3, return_resid=True)                      # the primal state is still there, and unchanged
        assert torch.equal(again[0], delta) and torch.equal(again[2], hist)
        assert (hist[1:, :, 2] > hist[:-1, :, 2]).all()                                       # ||delta|| grows at every round (CG from zero)
    assert eng.jac_lstsq(tap, c, 0.5, 0.1, 1e-5, 0)[2].shape == (1, 3, 4)                      # iters = 0: the init row alone


@pytest.mark.parametrize("kind,tap", K.CASES)
def test_one_iteration_is_parallel_to_inv_jac(kind, tap):
    _, _, x, _ = _model(kind)
    net = _net(kind)
    c = K.rhs(kind, tap)
    for b in range(3):
        cb = None if _ctx(kind) is None else _ctx(kind)[b:b + 1]
        kw = dict(encoder_hidden_states=cb, op=tap[0], block_idx=tap[1])
        delta, info = net.jac_lstsq(x=x[b:b + 1].to(_dev()), t=TS[b], u=c[b], iters=1, **kw)
        v = net.inv_jac_zt(x[b:b + 1].to(_dev()), TS[b], cb, op=tap[0], block_idx=tap[1], u=c[b].to(_dev()))
        cos = float((delta.double() * v.double()).sum() / (delta.double().norm() * v.double().norm()))
        assert abs(cos) >= 1 - 1e-6 and cos < 0, (b, cos)                                       # inv_jac_* keeps the reference's sign
        assert int(info["iterations"][0]) == 1 and tuple(info["gamma"].shape) == (1, 2)


@pytest.mark.parametrize("regime", ["fixed", "converged"])
@pytest.mark.parametrize("kind,tap", K.CASES)
def test_accuracy_against_the_float64_restatement_and_the_dense_solve(kind, tap, regime):
    _, _, x, _ = _model(kind)
    bars = K.solve_bars(kind, tap, regime)
    kw = K.REGIMES[regime]
    if regime == "converged":
        assert bars["d64"] <= 4e-6, bars["d64"]                                                # the condition: float64 CGLS has reached the dense solution
        assert (bars["hist64"][-1, :, 3] == 1).all()
    net = _net(kind)
    delta, info = net.jac_lstsq(x=x.to(_dev()), t=TS, u=torch.from_numpy(bars["c"]).T.contiguous(), damping=0.0, mu=bars["mu"], iters=kw["iters"],
                                tol=kw["tol"], encoder_hidden_states=_ctx(kind), op=tap[0], block_idx=tap[1])
    got = K.rel_rows(delta.cpu().numpy(), bars["want"])
    print(f"{kind} {tap} {regime}: float32 oracle {bars['d32']:.3e}, device {got:.3e} ({got / bars['d32']:.2f} d), float64 to dense {bars['d64']:.3e}, "
          f"iterations device {info['iterations'].tolist()} float64 {(bars['hist64'][:, :, 3] == 0).sum(0).tolist()}")
    assert got <= 8 * bars["d32"], (got, bars["d32"])
    assert torch.allclose(info["mu"].cpu(), torch.full((3,), bars["mu"], dtype=torch.float64), rtol=1e-12)
    if regime == "converged":
        assert info["converged"].all() and (info["iterations"] <= 32).all() and (info["iterations"] > 1).all()
    else:
        assert not info["converged"].any() and (info["iterations"] == 8).all()
        # the norms of the history against the float64 restatement's: an fp32 solve is ~1e-6 from it, a wrong step O(1)
        h64 = bars["hist64"]
        assert np.allclose(info["resid_norm"].cpu().numpy().T, np.sqrt(h64[:, :, 1]), rtol=1e-4)
        assert np.allclose(info["delta_norm"].cpu().numpy().T, np.sqrt(h64[:, :, 2]), rtol=1e-4)


def test_rows_and_flags_of_the_python_surface():
    kind, tap = "ddpm", ("mid", 0)
    _, _, x, _ = _model(kind)
    net = _net(kind)
    c = K.rhs(kind, tap)
    xd = x.to(_dev())
    kw = dict(op=tap[0], block_idx=tap[1], iters=4)
    # one sample, k right-hand sides: row i is the solve of column i alone (another batch of tangents: close, not bitwise)
    many, info = net.jac_lstsq(x=xd[:1], t=TS[0], u=c.T.contiguous(), **kw)
    assert many.shape == (3, x[0].numel()) and info["gamma"].shape == (3, 5)
    for i in range(3):
        one, _ = net.jac_lstsq(x=xd[:1], t=TS[0], u=c[i], **kw)
        assert K.rel_rows(one.cpu().numpy(), many[i:i + 1].cpu().numpy()) <= 1e-4
    # more right-hand sides than max_rank: chunks
    five, _ = net.jac_lstsq(x=xd[:1], t=TS[0], u=torch.cat([c, c[:2]]).T.contiguous(), **kw)
    assert five.shape[0] == 5 and K.rel_rows(five[3:].cpu().numpy(), many[:2].cpu().numpy()) <= 1e-4
    # a zero right-hand side converges at once (flag 1, delta = 0); a NaN one is named, or returned with check=False
    z = c.clone(); z[1] = 0
    delta, info = net.jac_lstsq(x=xd, t=TS, u=z.T.contiguous(), **kw)
    assert info["converged"].tolist() == [False, True, False] and info["iterations"].tolist() == [4, 0, 4] and (delta[1] == 0).all()
    z[1, 7] = float("nan")
    with pytest.raises(ValueError, match="row 1 .* the start"):
        net.jac_lstsq(x=xd, t=TS, u=z.T.contiguous(), **kw)
    delta, info = net.jac_lstsq(x=xd, t=TS, u=z.T.contiguous(), check=False, **kw)
    assert torch.isnan(delta[1]).all() and torch.isfinite(delta[[0, 2]]).all() and info["flag"].tolist() == [0, 3, 0]
    with pytest.raises(ValueError, match="one right-hand side per sample"):
        net.jac_lstsq(x=xd, t=TS, u=c[:2].T.contiguous(), **kw)
    with pytest.raises(ValueError, match="damping"):
        net.jac_lstsq(x=xd, t=TS, u=c.T.contiguous(), damping=-1.0, **kw)


def test_error_paths_leave_a_message_and_the_state_usable():
    from diffusion_pullback_amd import lib as L
    kind, tap = "ddpm", ("mid", 0)
    _, _, x, _ = _model(kind)
    net = _net(kind)
    eng = net.engine
    c = K.rhs(kind, tap).to(_dev())
    eng.forward(x.to(_dev()), TS, None, tap)                                                   # leaves no primal state
    with pytest.raises(L.DpbError):
        eng.jac_lstsq(tap, c)
    eng.primal(x.to(_dev()), TS, None, tap)
    ref = eng.jac_lstsq(tap, c, 0.0, 0.1, 1e-5, 2)
    for kw, word in ((dict(mu_abs=-1.0), "mu_abs"), (dict(mu_rel=float("inf")), "mu_rel"), (dict(tol=float("nan")), "tol"), (dict(iters=-1), "iters=-1")):
        with pytest.raises(L.DpbError, match=word):
            eng.jac_lstsq(tap, c, **kw)
    with pytest.raises(L.DpbError):                                                            # four rows for three samples
        eng.jac_lstsq(tap, torch.cat([c, c[:1]]))
    lib, buf = L.load(), eng.tape.taps[tap]
    need = int(lib.dpb_jac_lstsq_scratch_bytes(eng.h, buf, 3))
    assert need > 0 and lib.dpb_jac_lstsq_scratch_bytes(eng.h, -1, 3) == 0 and lib.dpb_jac_lstsq_scratch_bytes(eng.h, buf, 0) == 0
    sc = torch.empty(need + 512, dtype=torch.uint8, device=_dev())
    base = sc.data_ptr() + (-sc.data_ptr()) % 256
    delta = torch.empty(3, x[0].numel(), device=_dev())
    hist = torch.empty(3, 3, 4, dtype=torch.float64, device=_dev())
    call = lambda scratch=base, nbytes=need, tap_buf=buf: lib.dpb_jac_lstsq(eng.h, tap_buf, c.data_ptr(), 3, 0.0, 0.1, 1e-5, 2, delta.data_ptr(), None,
                                                                            hist.data_ptr(), C.c_void_p(scratch), nbytes)
    for kw, word in ((dict(nbytes=need - 1), b"scratch of"), (dict(scratch=base + 8), b"aligned"), (dict(tap_buf=10 ** 6), b"")):
        assert call(**kw) != 0 and word in lib.dpb_last_error(), (kw, lib.dpb_last_error())
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(delta, ref[0]) and torch.equal(hist, ref[2])
