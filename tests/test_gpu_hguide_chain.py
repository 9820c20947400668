"""PullbackUNet.h_space_guidance (dpb_hguide_chain) on the toy DDPM, ADM and SD nets of tests/test_gpu_inv_jac_chain.py (side 8): consistency with the
engine's own grouped pass and step, and accuracy against the float64 chain of tests/_hguide_ref.py on the oracle's CPU nets.

3 chains x 3 steps, the steps 30 .. 32 of the 100-step table (t = 696.27, 686.18, 676.09), directions 0, 1, 1 of two random unit directions, scales
0, 20, -30 (a unit direction of N_h elements moves each by scale / sqrt(N_h): of the size of the activations), mode asyrp unless stated.

The accuracy bars are measured on the reference side only (_bars), by the rule of tests/test_gpu_inv_jac_chain.py: the oracle chain runs in float32 and
in float64 on the CPU; d_step is their worst one-step difference with every step started from the float64 chain's state, d_chain their worst
free-running difference -- states absolute, delta_norm relative (over the chains with a shift).  The device must stay within 8 d: it differs from the
CPU float32 run in summation order only.  ADM: tests/_adm_ref.py restates the middle block's tap, so ADM mid is a case too; its other taps are held by
the consistency test alone.
Measured d (states / delta_norm) and the device's worst ratio to them, one MI355X run (the test prints them at every run):
  net, tap       d_step (states, delta_norm)   d_chain (states, delta_norm)  device / d, worst
  ddpm mid 0     2.4e-06  9.5e-07           3.9e-06  5.3e-07           1.06
  ddpm down 1    2.8e-06  3.2e-07           4.3e-06  3.2e-07           2.30
  ddpm up 1      2.3e-06  6.8e-07           4.6e-06  4.4e-07           1.25
  adm mid 0      2.4e-06  3.4e-07           4.4e-06  4.3e-07           1.07
  sd mid 0       4.6e-06  6.4e-06           5.8e-06  4.0e-06           1.06
  sd down 0      4.8e-06  1.8e-06           6.3e-06  1.3e-06           1.05
  sd up 1        5.0e-06  6.4e-06           6.4e-06  6.4e-06           1.02
(the CPU's float32 summation order moves d by a factor of two or so from run to run; the scale-0 chain equalled the plain unet + scheduler.step loop bit for bit.)
"""
import functools

import pytest
import torch

import _hguide_ref as R
import test_gpu_inv_jac_chain as IJ

pytestmark = pytest.mark.gpu

F32, BF, F16 = torch.float32, torch.bfloat16, torch.float16
DIRS, SCALES = [0, 1, 1], [0.0, 20.0, -30.0]
U_SEED = 34
KEYS = ("states", "delta_norm")
CASES = [("ddpm", ("mid", 0)), ("ddpm", ("down", 1)), ("ddpm", ("up", 1)), ("adm", ("mid", 0)), ("sd", ("mid", 0)), ("sd", ("down", 0)), ("sd", ("up", 1))]


@functools.lru_cache(maxsize=None)
def _table():
    from diffusion_pullback_amd.scheduler import YHCustomScheduler
    s = YHCustomScheduler(noise_schedule="linear")
    s.set_timesteps(100)
    return s.ddim_triples(30, 33)


def _u(n_h):
    return torch.randn(n_h, 2, generator=torch.Generator().manual_seed(U_SEED))


def _run(net, tap, x, ctx, u, scales=SCALES, mode="asyrp", table=None, **kw):
    ts, al, an = table or _table()
    dev = IJ._dev()
    return net.h_space_guidance(x=x.to(dev), timesteps=ts, alphas=al, alphas_next=an, u=u, dirs=DIRS, scales=scales, mode=mode,
                                encoder_hidden_states=None if ctx is None else ctx.to(dev), op=tap[0], block_idx=tap[1], **kw)


def _dist(a, b, key):
    d = (a[key].double().cpu() - b[key].double().cpu()).abs()
    if key == "states":
        return float(d.max())
    return float((d[1:] / b[key].double().cpu()[1:]).max())            # chain 0 has no shift: its delta is 0 on both sides


@functools.lru_cache(maxsize=None)
def _bars(kind, tap, mode=(1.0, 0.0)):
    """(ref64, resync64, d_step, d_chain): the float64 chain, its one-step restatement, and the float32 oracle's distances from both"""
    cfg, p, x, ctx = IJ._model(kind)
    ts, al, an = _table()
    n64, n32 = R.nets(kind, cfg, p, ctx, tap, torch.float64), R.nets(kind, cfg, p, ctx, tap, torch.float32)
    with torch.no_grad():
        u = _u(_n_h(kind, cfg, p, x, ctx, tap))
    c = torch.stack([u[:, d] / u[:, d].norm() for d in DIRS])
    ref64 = R.chain_ref(n64, x, c, SCALES, ts, al, an, *mode, torch.float64)
    ref32 = R.chain_ref(n32, x, c, SCALES, ts, al, an, *mode, torch.float32)
    rs64 = R.resync_ref(n64, ref64, c, SCALES, ts, al, an, *mode, torch.float64)
    rs32 = R.resync_ref(n32, ref64, c, SCALES, ts, al, an, *mode, torch.float32)
    cut = lambda r: {"states": r["states"][:, 1:], "delta_norm": r["delta_norm"]}
    return ref64, rs64, {k: _dist(rs32, rs64, k) for k in KEYS}, {k: _dist(cut(ref32), cut(ref64), k) for k in KEYS}, u


def _n_h(kind, cfg, p, x, ctx, tap):
    """elements of the tap, from the oracle's get_h"""
    if kind == "sd":
        from oracle import unet_sd
        return unet_sd.forward(p, cfg, x[:1], torch.tensor(1.0), ctx[:1], stop=tap).numel()
    if kind == "ddpm":
        from oracle import unet_ddpm
        return unet_ddpm.forward(p, cfg, x[:1], torch.tensor(1.0), stop=tap).numel()
    return IJ.A.get_h(p, cfg, x[:1], 1.0).numel()


@pytest.mark.parametrize("kind,tap", CASES)
def test_accuracy_against_the_float64_chain(kind, tap):
    """free-running within 8 d_chain, re-synchronised within 8 d_step; the scale-0 chain is the plain unet + scheduler.step loop within d_chain's bar"""
    _, _, x, ctx = IJ._model(kind)
    ref64, rs64, d_step, d_chain, u = _bars(kind, tap)
    net = IJ._net(kind, max_batch=6)
    ts, al, an = _table()
    free = _run(net, tap, x, ctx, u)
    cut = lambda r: {"states": r["states"][:, 1:], "delta_norm": r["delta_norm"]}
    rs = {"states": [], "delta_norm": []}
    for j in range(len(ts)):
        r = _run(net, tap, ref64["states"][:, j].float(), ctx, u, table=(ts[j:j + 1], al[j:j + 1], an[j:j + 1]))
        rs["states"].append(r["states"][:, 1].cpu()); rs["delta_norm"].append(r["delta_norm"][:, 0].cpu())
    rs = {k: torch.stack(v, dim=1) for k, v in rs.items()}
    got_step, got_chain = {k: _dist(rs, rs64, k) for k in KEYS}, {k: _dist(cut(free), cut(ref64), k) for k in KEYS}
    print(f"{kind} {tap}: d_step " + " ".join(f"{k} {d_step[k]:.3e}" for k in KEYS) + " | d_chain " + " ".join(f"{k} {d_chain[k]:.3e}" for k in KEYS))
    print("   device:  step " + " ".join(f"{k} {got_step[k]:.3e}" for k in KEYS) + " | chain " + " ".join(f"{k} {got_chain[k]:.3e}" for k in KEYS)
          + f" | worst ratio {max(max(got_step[k] / d_step[k], got_chain[k] / d_chain[k]) for k in KEYS):.2f}")
    for k in KEYS:
        assert got_step[k] <= 8 * d_step[k], (k, got_step[k], d_step[k])
        assert got_chain[k] <= 8 * d_chain[k], (k, got_chain[k], d_chain[k])
    assert float(ref64["delta_norm"][1:].min()) > 1e-3 and float(ref64["delta_norm"][0].max()) < 1e-9   # the shifts are no rounding-size change of eps
    # dx_norm is the coefficient times delta_norm
    coef = torch.stack([R.dx_coef(a, a2, 1.0, 0.0).abs() for a, a2 in zip(al, an)])
    assert torch.allclose(free["dx_norm"].cpu(), free["delta_norm"].cpu() * coef, rtol=1e-12, atol=0)
    # the scale-0 chain against the plain loop: unet + scheduler.step, one sample
    from diffusion_pullback_amd.scheduler import YHCustomScheduler
    s = YHCustomScheduler(noise_schedule="linear")
    s.set_timesteps(100)
    dev = IJ._dev()
    cur, c0 = x[:1].to(dev), None if ctx is None else ctx[:1].to(dev)
    for i in range(30, 33):
        e = net(cur, s.timesteps[i], c0)
        cur = s.step(e.sample if kind == "sd" else e, s.timesteps[i], cur, eta=0).prev_sample
    gap = float((cur[0].cpu() - free["states"][0, -1].cpu()).abs().max())
    print(f"   scale 0 against the plain loop: {gap:.3e} (bar {8 * d_chain['states']:.3e})")
    assert gap <= 8 * d_chain["states"]


@pytest.mark.parametrize("dtype", [F32, BF, F16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("kind", ["ddpm", "adm", "sd"])
def test_chain_is_the_composition_bitwise(kind, dtype):
    """states and delta of the chain equal, bit for bit, forward_shift_groups (groups = 2, group 0 unshifted) + ddim_step_asym step by step on the same
    engine: fp32 at every tap, the 16-bit engines at the middle block; both modes"""
    from diffusion_pullback_amd import engine as E
    _, _, x, ctx = IJ._model(kind)
    net = IJ._net(kind, dtype, max_batch=6)
    eng = net.engine
    ts, al, an = _table()
    dev = IJ._dev()
    n = x.shape[0]
    cd = None if ctx is None else ctx.to(dev)
    for tap in (IJ._taps(net) if dtype == F32 else [("mid", 0)]):
        u = _u(eng.tap_numel(tap))
        U = (u / u.norm(dim=0, keepdim=True)).T.contiguous().to(dev)
        for gP, gD in ((1.0, 0.0), (1.0, 1.0)):
            states, delta = eng.hguide_chain(x.to(dev), ts, al, an, cd, tap, U, DIRS, SCALES, gP, gD)
            assert torch.equal(states[0].cpu(), x)
            cur = x.to(dev)
            for j in range(len(ts)):
                out = eng.forward_shift_groups(cur, 2, ts[j], cd, tap, U, [-1] * n + DIRS, [0.0] * n + SCALES)
                nxt, _, st = E.ddim_step_asym(cur.reshape(n, -1).contiguous(), out[:n].reshape(n, -1), out[n:].reshape(n, -1), al[j], an[j], gP, gD)
                assert torch.equal(nxt.view_as(cur), states[j + 1]) and torch.equal(st, delta[j]), (tap, gP, gD, j)
                cur = nxt.view_as(cur)
            assert torch.isfinite(states).all() and (delta[..., 1] == 0).all() and (delta[:, 1:, 0] > 0).all()
        again = eng.hguide_chain(x.to(dev), ts, al, an, cd, tap, U, DIRS, SCALES, 1.0, 1.0)
        assert torch.equal(again[0], states) and torch.equal(again[1], delta), tap


@pytest.mark.parametrize("kind", ["ddpm", "sd"])
def test_zero_g_is_independent_of_the_shift_and_modes_differ(kind):
    """g = (0, 0): the states are bitwise those of any other u, dir and scale (the plain DDIM chain); asyrp and symmetric differ; a single context row
    is expanded; chains beyond max_batch // 2 run in groups with the same bits"""
    _, _, x, ctx = IJ._model(kind)
    net = IJ._net(kind, max_batch=6)
    tap = ("mid", 0)
    u = _u(net.engine.tap_numel(tap))
    a = _run(net, tap, x, ctx, u, mode=(0.0, 0.0))
    b = net.h_space_guidance(x=x.to(IJ._dev()), timesteps=_table()[0], alphas=_table()[1], alphas_next=_table()[2], u=2.0 * u.flip(1), dirs=[1, 0, 0],
                             scales=[5.0, -1.0, 0.0], mode=(0.0, 0.0), encoder_hidden_states=None if ctx is None else ctx.to(IJ._dev()), op="mid", block_idx=0)
    assert torch.equal(a["states"], b["states"]) and (a["dx_norm"] == 0).all()
    asy, sym = _run(net, tap, x, ctx, u), _run(net, tap, x, ctx, u, mode="symmetric")
    assert float((asy["states"][0] - sym["states"][0]).abs().max()) < 1e-5                              # no shift: the same chain
    assert float((asy["states"][1:, -1] - sym["states"][1:, -1]).abs().max()) > 1e-4
    assert asy["states"].shape == (3, 4, *x.shape[1:]) and asy["delta_norm"].shape == (3, 3) and asy["dx_norm"].shape == (3, 3)
    small = IJ._net(kind, max_batch=2)                                   # one chain per call
    one = _run(small, tap, x, ctx, u)
    assert torch.allclose(one["states"], asy["states"], atol=1e-5, rtol=1e-4)
    if ctx is not None:
        same = _run(net, tap, x, ctx[:1].expand(3, -1, -1).contiguous(), u)
        assert torch.equal(_run(net, tap, x, ctx[:1], u)["states"], same["states"])


def test_error_paths_leave_a_message_and_the_next_call_is_unaffected():
    from diffusion_pullback_amd import DpbError
    _, _, x, ctx = IJ._model("sd")
    net = IJ._net("sd", max_batch=6)
    eng = net.engine
    tap = ("mid", 0)
    ts, al, an = _table()
    dev = IJ._dev()
    u = _u(eng.tap_numel(tap))
    U = (u / u.norm(dim=0, keepdim=True)).T.contiguous().to(dev)
    xd, cd = x.to(dev), ctx.to(dev)
    good = eng.hguide_chain(xd, ts, al, an, cd, tap, U, DIRS, SCALES)
    call = lambda **k: eng.hguide_chain(k.get("x", xd), k.get("ts", ts), k.get("al", al), k.get("an", an), k.get("ctx", cd), k.get("tap", tap), k.get("U", U),
                                        k.get("dirs", DIRS), k.get("scales", SCALES), k.get("gP", 1.0), k.get("gD", 0.0))
    x4 = torch.cat([xd, xd[:1]])
    c4 = torch.cat([cd, cd[:1]])
    for kw, word in ((dict(x=x4, ctx=c4, dirs=DIRS + [0], scales=SCALES + [0.0]), "max_batch"), (dict(ts=[], al=[], an=[]), "steps=0"),
                     (dict(dirs=[0, 2, 1]), r"dir\[1\]=2"), (dict(dirs=[-1, 0, 1]), r"dir\[0\]=-1"), (dict(scales=[0.0, float("inf"), 1.0]), r"scale\[1\]"),
                     (dict(ts=[ts[0], float("nan"), ts[2]]), r"t\[1\]"), (dict(gP=float("nan")), "not finite"), (dict(gD=float("inf")), "not finite"),
                     (dict(al=[al[0], 0.0, al[2]]), r"\(0, 1\]"), (dict(an=[1.5, an[1], an[2]]), r"\(0, 1\]"), (dict(tap="eps", U=torch.zeros(2, eng.tap_numel("eps"))), "not downstream")):
        with pytest.raises(DpbError, match=word):
            call(**kw)
    with pytest.raises(DpbError):                                        # a missing context
        eng.hguide_chain(xd, ts, al, an, None, tap, U, DIRS, SCALES)
    temb = eng.tape.temb_in                                              # a buffer that does not depend on x is no tap to shift
    eng.tape.taps["temb"] = temb; eng.tape.tap_shape[temb] = (eng.tape.buffers[temb][1], 1, 1)
    try:
        with pytest.raises(DpbError, match="does not depend on x|invalid tap buffer"):
            eng.hguide_chain(xd, ts, al, an, cd, "temb", torch.zeros(1, eng.tap_numel("temb"), device=dev), [0, 0, 0], SCALES)
    finally:
        del eng.tape.taps["temb"], eng.tape.tap_shape[temb]
    # scratch too small or misaligned, through the C entry point
    import ctypes as C
    L = eng.lib
    fa = (C.c_float * 3)
    states = torch.empty(4, *xd.shape, device=dev)
    delta = torch.empty(3, 3, 2, dtype=torch.float64, device=dev)
    need = int(L.dpb_hguide_chain_scratch_bytes(eng.h, 3, 3))
    sc = torch.empty(need + 512, dtype=torch.uint8, device=dev)
    off = (-sc.data_ptr()) % 256
    args = lambda p, b: (eng.h, eng.tape.taps[tap], eng.tape.taps["eps"], xd.data_ptr(), 3, fa(*ts), fa(*al), fa(*an), cd.data_ptr(), U.data_ptr(), 2,
                         (C.c_int32 * 3)(*DIRS), fa(*SCALES), 1.0, 0.0, 3, states.data_ptr(), delta.data_ptr(), C.c_void_p(p), b)
    assert need > 0 and L.dpb_hguide_chain(*args(sc.data_ptr() + off, need - 1)) != 0 and b"scratch" in L.dpb_last_error()
    assert L.dpb_hguide_chain(*args(sc.data_ptr() + off + 8, need)) != 0 and b"aligned" in L.dpb_last_error()
    assert L.dpb_hguide_chain(*args(sc.data_ptr() + off, need)) == 0 and torch.equal(states, good[0]) and torch.equal(delta, good[1])
    with pytest.raises(DpbError):                                        # no primal state is left behind
        eng.jvp(tap, torch.zeros(1, eng.n_in, device=dev))
    with pytest.raises(ValueError, match="mode"):
        _run(net, tap, x, ctx, u, mode="other")
    with pytest.raises(ValueError, match="dirs"):
        net.h_space_guidance(x=xd, timesteps=ts, alphas=al, alphas_next=an, u=u, dirs=[0, 5, 1], scales=SCALES, encoder_hidden_states=cd, op="mid", block_idx=0)
    after = eng.hguide_chain(xd, ts, al, an, cd, tap, U, DIRS, SCALES)
    assert torch.equal(after[0], good[0]) and torch.equal(after[1], good[1])
