"""PullbackUNet.inv_jac_chain (dpb_inv_jac_chain) on the toy DDPM, ADM and SD nets: consistency with the engine's own passes, and accuracy against
the float64 chain of tests/_chain_ref.py on the oracle's CPU nets.

The accuracy bars are measured on the reference side only (_bars): the oracle chain runs in float32 and in float64 on the CPU; d_step is their
worst one-step difference with every step started from the float64 chain's state, d_chain their worst free-running difference, the states'
normalised by the step size s.  The device must stay within 8 d: it differs from the CPU float32 run in summation order only, a wrong direction is
an O(1) error.  The same rule for norm (relative), h_shift and h_dist (absolute, normalised by s).
Measured d (states / norm / h_shift / h_dist; 3 chains x 3 steps of s = 0.5, per-sample timesteps; the test prints them, and the device's
distances beside them, at every run -- they move by a factor of two or so with the CPU's own float32 summation order):
  net, tap       d_step (no SEGA)                             d_chain (no SEGA)                            device / d, worst
  ddpm mid 0     6.8e-07  3.1e-07  2.9e-06  1.5e-05           1.6e-06  6.3e-07  8.3e-06  3.6e-05           3.8
  ddpm down 1    2.9e-07  1.6e-07  4.3e-06  6.3e-06           4.7e-07  1.6e-07  2.6e-06  8.2e-06           2.6
  ddpm up 1      5.0e-07  3.5e-07  4.3e-06  2.5e-05           1.1e-06  3.5e-07  8.4e-06  3.4e-05           1.6
  adm mid 0      2.6e-07  8.8e-08  3.7e-06  8.8e-06           7.0e-07  1.4e-07  4.3e-06  1.1e-05           1.2
  sd mid 0       8.7e-07  4.4e-07  4.1e-05  2.0e-04           8.7e-07  5.3e-07  4.1e-05  1.3e-04           2.1
  sd down 0      4.7e-07  5.3e-07  1.1e-05  8.1e-05           5.6e-07  5.3e-07  1.6e-05  6.2e-05           3.4
  sd up 1        6.1e-07  3.2e-07  1.4e-04  1.1e-03           1.3e-06  9.9e-07  2.6e-04  8.8e-04           2.7
With the SEGA rule (sigma = 1) the figures are of the same size (states 2.3e-07 .. 8.7e-07 per step, 5.2e-07 .. 9.0e-07 free-running)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _adm_ref as A
import _chain_ref as R
from _util import load_golden

pytestmark = pytest.mark.gpu

F32, BF, F16 = torch.float32, torch.bfloat16, torch.float16
S, STEPS, SIDE = 0.5, 3, 8
TS = [696.2727, 301.0, 17.5]
SIGNS = [1.0, -1.0, 1.0]
DIRS = [0, 1, 1]
# The directions' seed.  Under the SEGA rule an element of v at its threshold is cut in one run and kept in another -- an O(1 / sqrt(N)) jump that says
# nothing about either run -- so the seed is one for which the FLOAT64 chain keeps every element at least 1e-4 (relative) away from its threshold in
# every case below (asserted in _bars, on the CPU; fp32 moves an element by about 1e-5): the first of the seeds 1, 2, ... that does, with 2.3e-4.
# (Seed 11 puts an element 3e-6 from its threshold in the SD mid case, and the device and the float32 oracle then disagree about it.)
U_SEED = 34
SEGA_MARGIN = 1e-4


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return "cuda:0"


@functools.lru_cache(maxsize=None)
def _model(kind):
    """(cfg, fp32 params, x [3, ...], ctx [3, L, D] or None) of the toy nets of tests/test_gpu_timesteps.py (side 8) and the ADM toy T3"""
    g = torch.Generator().manual_seed(5)
    if kind == "sd":
        from oracle import unet_sd
        f = load_golden("pullback_zt_tiny.pt")
        cfg = unet_sd.SDConfig(**{**f["cfg"], "sample_size": SIDE})
        return cfg, unet_sd.init_params(cfg, seed=f["seed"], gain=f["gain"]), torch.randn(3, 4, SIDE, SIDE, generator=g), torch.randn(3, 5, 16, generator=g)
    if kind == "ddpm":
        from oracle import unet_ddpm
        f = load_golden("ddpm_small.pt")
        cfg = unet_ddpm.DDPMConfig(**{**f["cfg"], "resolution": SIDE, "attn_resolutions": (SIDE // 2,)})
        return cfg, unet_ddpm.init_params(cfg, seed=f["seed"]), torch.randn(3, 3, SIDE, SIDE, generator=g), None
    from diffusion_pullback_amd import configs as cf
    cfg = A.TOYS["T3"]
    return cfg, cf.adm_init_params(cfg, **A.init_kwargs(A.TOY_INIT["T3"])), torch.randn(3, 3, cfg.image_size, cfg.image_size, generator=g), None


def _net(kind, dtype=F32, max_batch=3, max_rank=3):
    from diffusion_pullback_amd import PullbackUNet
    cfg, p, _, _ = _model(kind)
    return PullbackUNet(kind, cfg, p, dtype=dtype, device=_dev(), max_batch=max_batch, max_rank=max_rank, verbose=False)


def _taps(net):
    return [k for k in net.engine.tape.taps if isinstance(k, tuple)]


def _u(net, tap, k=2):
    g = torch.Generator().manual_seed(U_SEED)
    return torch.randn(net.engine.tap_numel(tap), k, generator=g)


def _chain(net, kind, tap, x, t, u, ctx=None, **kw):
    kw.setdefault("steps", STEPS); kw.setdefault("step_size", S)
    return net.inv_jac_chain(x=x.to(_dev()), t=t, u=u, encoder_hidden_states=None if ctx is None else ctx.to(_dev()), op=tap[0], block_idx=tap[1], **kw)


def _get_hs(kind, tap, dtype, ts):
    """one CPU get_h per chain, parameters in `dtype`, chain b at timestep ts[b] with its own context row"""
    cfg, p, _, ctx = _model(kind)
    p = {k: v.to(dtype) for k, v in p.items()}
    if kind == "sd":
        from oracle import unet_sd
        return [lambda a, b=b: unet_sd.forward(p, cfg, a, torch.tensor(ts[b]), ctx[b:b + 1].to(dtype), stop=tap) for b in range(len(ts))]
    if kind == "ddpm":
        from oracle import unet_ddpm
        emb = unet_ddpm.timestep_embedding

        def fwd(a, b):                                            # the oracle's sinusoid is fp32 whatever the parameters: cast it for the float64 run
            unet_ddpm.timestep_embedding = lambda t, d: emb(t, d).to(dtype)
            try:
                return unet_ddpm.forward(p, cfg, a, torch.tensor(ts[b]), stop=tap)
            finally:
                unet_ddpm.timestep_embedding = emb
        return [lambda a, b=b: fwd(a, b) for b in range(len(ts))]
    return [lambda a, b=b: A.get_h(p, cfg, a, ts[b]) for b in range(len(ts))]


KEYS = ("states", "norm", "h_shift", "h_dist")


def _dist(a, b, key):
    """how far two runs are apart in one quantity: states and the shifts absolute over s, the norm relative"""
    d = (a[key].double().cpu() - b[key].double().cpu()).abs()
    return float((d / b[key].double().cpu().abs()).max()) if key == "norm" else float(d.max()) / S


def _resync(run_one_step, ref64):
    """one-step runs started from the float64 chain's states: {key: [n, STEPS] of the step's results, the shifts those of the state reached}"""
    out = {k: [] for k in KEYS}
    for j in range(STEPS):
        r = run_one_step(ref64["states"][:, j].float())
        out["states"].append(r["states"][:, 1].double().cpu()); out["norm"].append(r["norm"][:, 0].double().cpu())
        out["h_shift"].append(r["h_shift"][:, 1].double().cpu()); out["h_dist"].append(r["h_dist"][:, 1].double().cpu())
    return {k: torch.stack(v, dim=1) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _bars(kind, tap, sega):
    """(ref64, resync64, d_step, d_chain): the float64 chain, its one-step restatement, and the float32 oracle's distances from both"""
    _, _, x, _ = _model(kind)
    n = x.shape[0]
    D = int(np.prod(_get_hs(kind, tap, torch.float64, TS)[0](x[:1].double()).shape))
    u = torch.randn(D, 2, generator=torch.Generator().manual_seed(U_SEED))
    c = torch.stack([SIGNS[b] * u[:, DIRS[b]] for b in range(n)])
    g64, g32 = _get_hs(kind, tap, torch.float64, TS), _get_hs(kind, tap, torch.float32, TS)
    ref64 = R.chain_ref(g64, x, c, STEPS, [S] * n, sega, torch.float64)
    assert float(ref64["sega_margin"].min()) >= SEGA_MARGIN, f"the float64 chain has an element {float(ref64['sega_margin'].min()):.2e} from its SEGA threshold: another U_SEED"
    ref32 = R.chain_ref(g32, x, c, STEPS, [S] * n, sega, torch.float32)
    one = lambda g, dt: (lambda xs: R.chain_ref(g, xs, c, 1, [S] * n, sega, dt))
    rs64, rs32 = _resync(one(g64, torch.float64), ref64), _resync(one(g32, torch.float32), ref64)
    return ref64, rs64, {k: _dist(rs32, rs64, k) for k in KEYS}, {k: _dist(ref32, ref64, k) for k in KEYS}


CASES = [("ddpm", ("mid", 0)), ("ddpm", ("down", 1)), ("ddpm", ("up", 1)), ("adm", ("mid", 0)), ("sd", ("mid", 0)), ("sd", ("down", 0)), ("sd", ("up", 1))]


@pytest.mark.parametrize("sega", [None, 1.0])
@pytest.mark.parametrize("kind,tap", CASES)
def test_accuracy_against_the_float64_chain(kind, tap, sega):
    """free-running within 8 d_chain, re-synchronised within 8 d_step, per-sample timesteps and contexts, both signs, two directions; with the SEGA
    rule the kept counts are those of the float64 chain (U_SEED keeps every element clear of its threshold)"""
    _, _, x, ctx = _model(kind)
    ref64, rs64, d_step, d_chain = _bars(kind, tap, sega)
    net = _net(kind)
    u = _u(net, tap)
    run = lambda xs, steps: _chain(net, kind, tap, xs, TS, u, ctx, dirs=DIRS, signs=SIGNS, steps=steps, sega_sigma=sega)
    free = run(x, STEPS)
    rs = _resync(lambda xs: run(xs, 1), ref64)
    print(f"{kind} {tap} sega={sega}: d_step " + " ".join(f"{k} {d_step[k]:.3e}" for k in KEYS) + " | d_chain " + " ".join(f"{k} {d_chain[k]:.3e}" for k in KEYS))
    got_step, got_chain = {k: _dist(rs, rs64, k) for k in KEYS}, {k: _dist(free, ref64, k) for k in KEYS}
    print("   device:  step " + " ".join(f"{k} {got_step[k]:.3e}" for k in KEYS) + " | chain " + " ".join(f"{k} {got_chain[k]:.3e}" for k in KEYS))
    for k in KEYS:
        assert got_step[k] <= 8 * d_step[k], (k, got_step[k], d_step[k])
        assert got_chain[k] <= 8 * d_chain[k], (k, got_chain[k], d_chain[k])
    assert (free["h_shift"][:, 1:] < 0).all()                      # the sign convention: every chain moves h against its c
    if sega:
        assert torch.equal(free["sega_kept"].cpu(), ref64["sega_kept"]) and (free["sega_kept"] < x[0].numel()).all()


@pytest.mark.parametrize("dtype", [BF, F16])
@pytest.mark.parametrize("kind,tap", [("ddpm", ("mid", 0)), ("adm", ("mid", 0)), ("sd", ("mid", 0))])
def test_16_bit_engines_keep_the_direction(kind, tap, dtype):
    """re-synchronised only: cos of every v_k to the float64 one >= 0.99, the project's 16-bit bar for vT"""
    _, _, x, ctx = _model(kind)
    ref64 = _bars(kind, tap, None)[0]
    net = _net(kind, dtype)
    u = _u(net, tap)
    for j in range(STEPS):
        r = _chain(net, kind, tap, ref64["states"][:, j].float(), TS, u, ctx, dirs=DIRS, signs=SIGNS, steps=1, return_vk=True)
        v, w = r["vk"][:, 0].double().cpu(), ref64["vk"][:, j]
        cos = (v * w).sum(-1) / (v.norm(dim=-1) * w.norm(dim=-1))
        assert (cos >= 0.99).all(), (j, cos)


@pytest.mark.parametrize("kind", ["ddpm", "adm", "sd"])
def test_consistency_at_every_tap(kind):
    """at every tap of the net: the first step is x + s inv_jac_xt(x, t, u); steps = S is bitwise S calls of steps = 1 fed with the states; a
    repeated call is bitwise equal; final_shift=False leaves NaN in the last shift and changes nothing else"""
    _, _, x, ctx = _model(kind)
    net = _net(kind)
    for tap in _taps(net):
        u = _u(net, tap)
        kw = dict(dirs=DIRS, signs=SIGNS, return_vk=True)
        r = _chain(net, kind, tap, x, TS[0], u, ctx, **kw)
        again = _chain(net, kind, tap, x, TS[0], u, ctx, **kw)
        assert all(torch.equal(r[k], again[k]) for k in r), tap
        assert torch.equal(r["states"][:, 0].cpu(), x) and torch.isfinite(r["states"]).all()
        assert (r["sega_kept"] == x[0].numel()).all() and (r["sega_std"] == 0).all() and (r["h_shift"][:, 0] == 0).all() and (r["h_dist"][:, 0] == 0).all()
        cur = x
        for j in range(STEPS):
            one = _chain(net, kind, tap, cur, TS[0], u, ctx, steps=1, **kw)
            for k in ("norm", "sega_std", "sega_kept"):
                assert torch.equal(one[k][:, 0], r[k][:, j]), (tap, j, k)
            assert torch.equal(one["vk"][:, 0], r["vk"][:, j]) and torch.equal(one["states"][:, 1], r["states"][:, j + 1]), (tap, j)
            if j == 0:
                assert torch.equal(one["h_shift"], r["h_shift"][:, :2]) and torch.equal(one["h_dist"], r["h_dist"][:, :2])
            cur = one["states"][:, 1].cpu()
        nf = _chain(net, kind, tap, x, TS[0], u, ctx, final_shift=False, **kw)
        assert torch.isnan(nf["h_shift"][:, -1]).all() and torch.isnan(nf["h_dist"][:, -1]).all()
        assert all(torch.equal(nf[k], r[k]) for k in ("states", "vk", "norm")) and torch.equal(nf["h_shift"][:, :-1], r["h_shift"][:, :-1])
        # the first step against inv_jac: one chain per call, the batch of inv_jac_zt itself
        for b in range(x.shape[0]):
            cb = ctx[b:b + 1].to(_dev()) if ctx is not None else None
            c = (SIGNS[b] * u[:, DIRS[b]]).to(_dev())
            v = net.inv_jac_zt(x[b:b + 1].to(_dev()), TS[0], cb, op=tap[0], block_idx=tap[1], u=c).reshape(-1).double().cpu()
            one = _chain(net, kind, tap, x[b:b + 1], TS[0], u, None if ctx is None else ctx[b:b + 1], dirs=[DIRS[b]], signs=[SIGNS[b]], steps=1)
            xb = x[b].reshape(-1).double()
            err = (one["states"][0, 1].reshape(-1).double().cpu() - (xb + S * v)).abs()
            assert (err <= 4 * 2.0 ** -24 * (xb.abs() + S * v.abs())).all(), (tap, b, float(err.max()))


@pytest.mark.parametrize("kind", ["ddpm", "sd"])
def test_per_sample_timesteps_and_groups(kind):
    """row b of a chain call at t = [t_0, t_1, t_2] is the chain run alone at t_b (another batch, other tiles: within the one-step bar 8 d_step);
    five chains on an engine of max_batch 3 run as groups of 3 and 2, bitwise the two calls"""
    tap = ("mid", 0)
    _, _, x, ctx = _model(kind)
    d_step = _bars(kind, tap, None)[2]
    net = _net(kind)
    u = _u(net, tap)
    het = _chain(net, kind, tap, x, TS, u, ctx, dirs=DIRS, signs=SIGNS, steps=1)
    for b in range(3):
        alone = _chain(net, kind, tap, x[b:b + 1], TS[b], u, None if ctx is None else ctx[b:b + 1], dirs=[DIRS[b]], signs=[SIGNS[b]], steps=1)
        for k in KEYS:
            assert _dist({k: het[k][b:b + 1]}, {k: alone[k]}, k) <= 8 * d_step[k], (b, k)
    # the timestep embeddings are uploaded in step 0 and stay resident across the adjoint passes: with DISTINCT timesteps, steps = S is still bitwise
    # S calls of steps = 1 fed with the states (a stale embedding row would move every later state)
    full = _chain(net, kind, tap, x, TS, u, ctx, dirs=DIRS, signs=SIGNS, return_vk=True)
    assert torch.equal(full["states"][:, 1], het["states"][:, 1])
    cur = x
    for j in range(STEPS):
        one = _chain(net, kind, tap, cur, TS, u, ctx, dirs=DIRS, signs=SIGNS, steps=1, return_vk=True)
        assert torch.equal(one["states"][:, 1], full["states"][:, j + 1]) and torch.equal(one["vk"][:, 0], full["vk"][:, j]), j
        assert torch.equal(one["norm"][:, 0], full["norm"][:, j])
        cur = one["states"][:, 1].cpu()
    same = _chain(net, kind, tap, x, TS[1], u, ctx, dirs=DIRS, signs=SIGNS, steps=1)
    assert not torch.equal(same["states"][0], het["states"][0]) and torch.equal(same["states"][1], het["states"][1])   # the timesteps do matter
    x5 = torch.cat([x, x[:2] + 0.1]); c5 = None if ctx is None else torch.cat([ctx, ctx[:2]])
    t5, d5, s5 = TS + [TS[0], TS[2]], DIRS + [1, 0], SIGNS + [-1.0, 1.0]
    r = _chain(net, kind, tap, x5, t5, u, c5, dirs=d5, signs=s5, step_size=[S, S, 2 * S, S, S / 2], return_vk=True)
    a = _chain(net, kind, tap, x5[:3], t5[:3], u, None if c5 is None else c5[:3], dirs=d5[:3], signs=s5[:3], step_size=[S, S, 2 * S], return_vk=True)
    b = _chain(net, kind, tap, x5[3:], t5[3:], u, None if c5 is None else c5[3:], dirs=d5[3:], signs=s5[3:], step_size=[S, S / 2], return_vk=True)
    assert r["states"].shape == (5, STEPS + 1, *x.shape[1:]) and r["vk"].shape == (5, STEPS, x[0].numel())
    assert all(torch.equal(r[k], torch.cat([a[k], b[k]])) for k in r)


def test_error_paths_leave_a_message_and_the_next_call_is_unaffected():
    from diffusion_pullback_amd import lib as L
    kind, tap = "ddpm", ("mid", 0)
    _, _, x, _ = _model(kind)
    net = _net(kind)
    eng, u = net.engine, _u(net, tap)
    ref = _chain(net, kind, tap, x, TS, u, dirs=DIRS, signs=SIGNS)
    U = u.T.contiguous().to(_dev())
    xd = x.to(_dev())
    key = tap

    def refused(word, xs=xd, t=TS, dirs=DIRS, signs=SIGNS, step=(S, S, S), steps=STEPS):
        with pytest.raises(L.DpbError) as e:
            eng.inv_jac_chain(xs, t, None, key, U, dirs, signs, step, steps)
        assert word in str(e.value), (word, str(e.value))
        assert word.encode() in L.load().dpb_last_error()

    refused("steps=0", steps=0)
    refused("dir[1]=2", dirs=[0, 2, 1])
    refused("dir[0]=-1", dirs=[-1, 0, 1])
    refused("sign[2]", signs=[1.0, 1.0, float("inf")])
    refused("step[0]", step=(float("nan"), S, S))
    refused("t[1]", t=[1.0, float("nan"), 2.0])
    big = torch.cat([xd, xd[:1]])
    refused("n=4", xs=big, t=TS + [1.0], dirs=DIRS + [0], signs=SIGNS + [1.0], step=(S,) * 4)
    # straight at the C entry point: the tap, nu, the scratch
    lib, n = L.load(), 3
    buf = eng.tape.taps[key]
    need = int(lib.dpb_inv_jac_chain_scratch_bytes(eng.h, buf, n))
    assert need > 0 and lib.dpb_inv_jac_chain_scratch_bytes(eng.h, -1, n) == 0 and lib.dpb_inv_jac_chain_scratch_bytes(eng.h, buf, 0) == 0
    sc = torch.empty(need + 512, dtype=torch.uint8, device=_dev())
    base = sc.data_ptr() + (-sc.data_ptr()) % 256
    states = torch.empty(STEPS + 1, n, *x.shape[1:], device=_dev())
    stats = torch.empty(STEPS, n, 4, dtype=torch.float64, device=_dev())
    shift = torch.empty(STEPS + 1, n, 2, dtype=torch.float64, device=_dev())
    fa = lambda v: (C.c_float * n)(*v)

    def call(tap_buf=buf, nu=2, scratch=base, nbytes=need):
        return lib.dpb_inv_jac_chain(eng.h, tap_buf, xd.data_ptr(), n, fa(TS), None, U.data_ptr(), nu, (C.c_int32 * n)(*DIRS), fa(SIGNS), fa([S] * n), STEPS,
                                     0.0, 1, states.data_ptr(), None, stats.data_ptr(), shift.data_ptr(), C.c_void_p(scratch), nbytes)

    for kw, word in ((dict(tap_buf=eng.tape.temb_in), b"tap buffer"), (dict(tap_buf=10 ** 6), b"tap buffer"), (dict(nu=0), b"nu=0"),
                     (dict(nbytes=need - 1), b"scratch of"), (dict(scratch=base + 8), b"aligned")):
        assert call(**kw) != 0 and word in lib.dpb_last_error(), (kw, lib.dpb_last_error())
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(states.transpose(0, 1).cpu(), ref["states"].cpu())
    with pytest.raises(L.DpbError):                                  # the call leaves no primal state, as dpb_forward
        eng.vjp(key, torch.zeros(n, eng.tap_numel(key)))
    again = _chain(net, kind, tap, x, TS, u, dirs=DIRS, signs=SIGNS)
    assert all(torch.equal(again[k], ref[k]) for k in ref)
    # a chain that loses its direction: a zero u gives J^T c = 0 at the first step
    with pytest.raises(ValueError, match="chain 1 .* step 0"):
        _chain(net, kind, tap, x, TS, torch.stack([u[:, 0], torch.zeros_like(u[:, 0])], dim=1), dirs=DIRS, signs=SIGNS)
    r = _chain(net, kind, tap, x, TS, torch.stack([u[:, 0], torch.zeros_like(u[:, 0])], dim=1), dirs=[0, 1, 0], signs=SIGNS, check=False)
    assert torch.isnan(r["states"][1, 1:]).all() and torch.isfinite(r["states"][[0, 2]]).all()
