"""GPU tests of the h-space shifted forward: dpb_forward_shift (Engine.forward_shift) and its public surface -- PullbackUNet.__call__(x, t,
u=, op=, block_idx=) for DDPM, forward_dh for SD, h_traversal -- on the tiny SD net and the small DDPM net of tests/test_gpu_decoder.py, at
every tap (eps lies downstream of each of them).

Yardsticks: the reference's own PullBackDDPM.forward(x, t, u, op, block_idx) (tests/golden/make_golden_hshift.py: hshift_ddpm.pt) and the fp32
CPU restatement of get_h_to_e (tests/_decoder_ref.py) at input_h = h + scale * u, h from the CPU oracle's get_h.  Bars: rel < 2e-4 against the
restatement and the golden in fp32 (the bar of get_h_to_e in test_gpu_decoder.py and of the DDPM goldens in test_gpu_parity.py); atol 1e-5 /
rtol 1e-4 between two engine paths (test_gpu_decoder.py:234); first order rel < 2e-2 at a = 1e-3 (test_get_h_to_e_forward_and_first_order);
16 bit: 1.5 x the error of the existing get_h + get_h_to_e(h + s u) composition on the same engine and inputs."""
import functools

import pytest
import torch

from _decoder_ref import ddpm_h_to_e, sd_h_to_e
from _util import load_golden, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAPS = {"sd": [("down", 0), ("down", 1), ("mid", 0), ("up", 0), ("up", 1)],
        "ddpm": [("down", 0), ("down", 1), ("down", 2), ("mid", 0), ("up", 2), ("up", 1), ("up", 0)]}
DIRS, SCALES = [-1, 0, 1, 0], [0.0, 0.5, -2.0, 1.5]       # the rows of the shared-prefix calls (batch 3: the first three)


@functools.lru_cache(maxsize=None)
def _setup(kind):
    """net description, two distinct samples (row 0: the fixture's), two directions per tap scaled to the tap's spread, h of both samples"""
    g = torch.Generator().manual_seed(21)
    if kind == "sd":
        from oracle import unet_sd
        f = load_golden("decoder_zt_tiny.pt")
        cfg = unet_sd.SDConfig(**f["cfg"])
        p = unet_sd.init_params(cfg, seed=f["seed"], gain=f["gain"])
        x = torch.cat([f["z"], torch.randn(f["z"].shape, generator=g)])
        ctx = torch.cat([f["ctx"], torch.randn(f["ctx"].shape, generator=g)])
        t = f["t"]
        get_h = lambda b, tap: unet_sd.forward(p, cfg, x[b:b + 1], t, ctx[b:b + 1], stop=tap)
    else:
        from oracle import unet_ddpm
        f = load_golden("decoder_xt_ddpm.pt")
        cfg = unet_ddpm.DDPMConfig(**f["cfg"])
        p = unet_ddpm.init_params(cfg, seed=f["seed"])
        x = torch.cat([f["x"], torch.randn(f["x"].shape, generator=g)])
        ctx, t = None, f["t"]
        get_h = lambda b, tap: unet_ddpm.forward(p, cfg, x[b:b + 1], t, stop=tap)
    h, u = {}, {}
    with torch.no_grad():
        for tap in TAPS[kind]:
            h[tap] = [get_h(b, tap) for b in range(2)]
            u[tap] = 0.5 * h[tap][0].std() * torch.randn(2, h[tap][0].numel(), generator=g)
    return dict(cfg=cfg, p=p, x=x, ctx=ctx, t=t, h=h, u=u)


@functools.lru_cache(maxsize=None)
def _ref(kind, tap, b, d, s):
    """CPU restatement: eps of sample b with h_b + s * u_d at the tap (d = -1: unshifted), computed once per (tap, row)"""
    S = _setup(kind)
    hh = S["h"][tap][b] + (s * S["u"][tap][d].reshape(S["h"][tap][b].shape) if d >= 0 else 0.0)
    with torch.no_grad():
        if kind == "sd":
            return sd_h_to_e(S["p"], S["cfg"], S["x"][b:b + 1], S["t"], S["ctx"][b:b + 1], hh, *tap)
        return ddpm_h_to_e(S["p"], S["cfg"], S["x"][b:b + 1], S["t"], hh, *tap)


def _net(kind, dtype=torch.float32, max_batch=4, max_rank=2):
    from diffusion_pullback_amd import PullbackUNet
    S = _setup(kind)
    return PullbackUNet(kind, S["cfg"], S["p"], dtype=dtype, device=DEV, max_batch=max_batch, max_rank=max_rank, verbose=False)


def _ctx(S, rows):
    return None if S["ctx"] is None else S["ctx"][rows]


# ------------------------------------------------------------------------------------------------ 1. per-sample x
@pytest.mark.parametrize("kind", ["sd", "ddpm"])
def test_per_sample_rows_vs_restatement(kind):
    """xbatch = batch = 2, distinct x / ctx rows, dir = [1, 0], scale = [0.7, -1.3]: every row against the restatement at its own sample"""
    S = _setup(kind)
    e = _net(kind, max_batch=2).engine
    errs = {}
    for tap in TAPS[kind]:
        out = e.forward_shift(S["x"], float(S["t"]), S["ctx"], tap, S["u"][tap], [1, 0], [0.7, -1.3]).cpu()
        errs[tap] = [rel(out[b:b + 1], _ref(kind, tap, b, d, s)) for b, (d, s) in enumerate([(1, 0.7), (0, -1.3)])]
        assert rel(out[0:1], _ref(kind, tap, 0, -1, 0.0)) > 1e-3, tap      # (the shift is no rounding-size change of eps)
    print(kind, errs)
    assert all(max(v) < 2e-4 for v in errs.values()), errs


# ------------------------------------------------------------------------------------------------ 2. shared prefix
@pytest.mark.parametrize("batch", [3, 4], ids=["b3", "bmax"])
@pytest.mark.parametrize("kind", ["sd", "ddpm"])
def test_shared_prefix_vs_unet_restatement_and_repeated_x(kind, batch):
    S = _setup(kind)
    net = _net(kind, max_batch=4)
    e, t = net.engine, float(S["t"])
    x1, c1 = S["x"][0:1], _ctx(S, slice(0, 1))
    eps = net(x1, S["t"], c1)
    eps = (eps.sample if kind == "sd" else eps).cpu()
    dirs, scales = DIRS[:batch], SCALES[:batch]
    errs = {}
    for tap in TAPS[kind]:
        out = e.forward_shift(x1, t, c1, tap, S["u"][tap], dirs, scales).cpu()
        assert out.shape == (batch, *eps.shape[1:])
        assert torch.allclose(out[0:1], eps, atol=1e-5, rtol=1e-4), (tap, (out[0:1] - eps).abs().max())      # dir = -1: the plain forward
        errs[tap] = [rel(out[b:b + 1], _ref(kind, tap, 0, dirs[b], scales[b])) for b in range(1, batch)]
        rep = e.forward_shift(x1.expand(batch, -1, -1, -1), t, None if c1 is None else c1.expand(batch, -1, -1), tap, S["u"][tap], dirs, scales).cpu()
        assert torch.allclose(out, rep, atol=1e-5, rtol=1e-4), (tap, (out - rep).abs().max())
    print(kind, batch, errs)
    assert all(max(v) < 2e-4 for v in errs.values()), errs


# ------------------------------------------------------------------------------------------------ 3. first order
@pytest.mark.parametrize("kind", ["sd", "ddpm"])
def test_first_order_is_the_decoder_jvp(kind):
    S = _setup(kind)
    e = _net(kind, max_batch=2).engine
    x1, c1, t = S["x"][0:1], _ctx(S, slice(0, 1)), float(S["t"])
    g = torch.Generator().manual_seed(22)
    a = 1e-3
    errs = {}
    for tap in TAPS[kind]:
        d = torch.randn(1, e.tap_numel(tap), generator=g)
        out = e.forward_shift(x1, t, c1, tap, d, [-1, 0], [0.0, a]).cpu()
        e.primal(x1, t, c1, "eps")
        Jd = e.jvp_between(tap, "eps", d.to(DEV)).cpu().reshape(out[1].shape)
        errs[tap] = rel(out[1] - out[0], a * Jd)
    print(kind, errs)
    assert all(v < 2e-2 for v in errs.values()), errs


# ------------------------------------------------------------------------------------------------ 4. work actually shared
@pytest.mark.parametrize("kind", ["sd", "ddpm"])
def test_shared_prefix_flops_and_launches(kind):
    """F(tap, b): gemm_flops after forward to tap at batch b.  The shared-prefix call runs the prefix once: F(src, 1) + F(eps, B) - F(src, B),
    exactly -- the x-independent ops need no correction: the SHARED ones (timestep MLP, time-embedding projections) cost the same at any batch
    and appear once in each term, the context's K/V projection is per sample and lies in the prefix.  The launches follow the same identity, plus
    shift_tap and (where a later op reads an earlier buffer) replicate_rows."""
    S = _setup(kind)
    B = 4
    e = _net(kind, max_batch=B).engine
    x1, c1, t = S["x"][0:1], _ctx(S, slice(0, 1)), float(S["t"])
    xB, cB = x1.expand(B, -1, -1, -1), None if c1 is None else c1.expand(B, -1, -1)

    def stats(x, c, tap):
        e.forward(x, t, c, tap)
        n, fl, _ = e.stats()
        return n, fl
    nE, fE = stats(xB, cB, "eps")
    for tap in TAPS[kind]:
        n1, f1 = stats(x1, c1, tap)
        nB, fB = stats(xB, cB, tap)
        e.forward_shift(x1, t, c1, tap, S["u"][tap], DIRS, SCALES)
        n, fl, _ = e.stats()
        want = f1 + fE - fB
        print(kind, tap, "flops", fl, "of", fE, "launches", n, "of", nE)
        assert fl < fE, (tap, fl, fE)
        assert abs(fl - want) <= 1e-9 * want, (tap, fl, want)
        extra = 1 if tap == TAPS[kind][-1] else 2                         # (after the last up tap only norm_out + conv_out run: nothing to broadcast)
        assert n == n1 + (nE - nB) + extra, (tap, n, n1, nE, nB)
        e.forward_shift(xB, t, cB, tap, S["u"][tap], DIRS, SCALES)       # per-sample x: the whole pass at B, one more launch (shift_tap)
        n, fl, _ = e.stats()
        assert abs(fl - fE) <= 1e-9 * fE and n == nE + 1, (tap, n, nE, fl, fE)


def test_shared_prefix_more_rows_than_one_launch_carries():
    """xbatch = 1 and 66 rows on the small DDPM net (max_batch = 66): shift_tap carries 64 rows per launch, so the groups go in two chunks, rows
    64 and 65 first and the chunk with row 0 -- the source of every row -- last.  Rows 0 and 64 are unshifted: row 0 is its own source and is left
    alone, row 64 is a copy that has to be written.  Rows 0, 63, 64, 65 against the restatement, and one launch more than the 64-row call."""
    kind, tap, B = "ddpm", ("mid", 0), 66
    S = _setup(kind)
    e = _net(kind, max_batch=B).engine
    x1, t = S["x"][0:1], float(S["t"])
    dirs = [b % 3 - 1 for b in range(B)]                                 # -1, 0, 1, ...: row 0 unshifted
    scales = [0.25 * (b % 7 - 3) for b in range(B)]
    dirs[63], scales[63], dirs[64], dirs[65], scales[65] = 0, 1.5, -1, 1, -2.0
    e.forward_shift(x1, t, None, tap, S["u"][tap], dirs[:64], scales[:64])
    n64 = e.stats()[0]
    out = e.forward_shift(x1, t, None, tap, S["u"][tap], dirs, scales).cpu()
    n66 = e.stats()[0]
    errs = {b: rel(out[b:b + 1], _ref(kind, tap, 0, dirs[b], scales[b] if dirs[b] >= 0 else 0.0)) for b in (0, 63, 64, 65)}
    print(errs, n64, n66)
    assert out.shape[0] == B and all(v < 2e-4 for v in errs.values()), errs
    assert n66 == n64 + 1, (n64, n66)


# ------------------------------------------------------------------------------------------------ 5. 16-bit engines
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("kind", ["sd", "ddpm"])
def test_16bit_rows_no_worse_than_get_h_to_e_composition(kind, dtype):
    """Both paths round the shifted tap once to the engine dtype; the new one adds in fp32 first.  Bar per row: 1.5 x the error of
    get_h + get_h_to_e(input_h = h + s u) on the same engine and inputs; the pairs (new, composition) are printed."""
    S = _setup(kind)
    net = _net(kind, dtype, max_batch=3)
    e = net.engine
    x1, c1, t = S["x"][0:1], _ctx(S, slice(0, 1)), float(S["t"])
    dirs, scales = [0, 1, 0], [0.5, -2.0, 1.5]
    pairs, bad = {}, {}
    for tap in TAPS[kind]:
        u = S["u"][tap]
        new = e.forward_shift(x1, t, c1, tap, u, dirs, scales).cpu()
        h = e.forward(x1, t, c1, tap).cpu()
        hs = torch.cat([h + s * u[d].reshape(h.shape) for d, s in zip(dirs, scales)])
        old = e.forward_from(x1.expand(3, -1, -1, -1), t, c1, tap, hs).cpu()
        refs = [_ref(kind, tap, 0, d, s) for d, s in zip(dirs, scales)]
        pairs[tap] = [(rel(new[b:b + 1], refs[b]), rel(old[b:b + 1], refs[b])) for b in range(3)]
        bad.update({(tap, b): pr for b, pr in enumerate(pairs[tap]) if not pr[0] <= 1.5 * pr[1]})
    print(kind, dtype, {k: [(round(a, 5), round(b, 5)) for a, b in v] for k, v in pairs.items()})
    assert not bad, f"(new, composition) row errors with new > 1.5 x composition: {bad}"


# ------------------------------------------------------------------------------------------------ 6. public surface
@pytest.mark.parametrize("dtype", [torch.float32], ids=["fp32"])
def test_ddpm_call_with_u_vs_reference_golden(dtype):
    """PullBackDDPM.forward(x, t, u, op, block_idx) (diffusion.py:145-200) through unet(x, t, u=, op=, block_idx=): B = 1 and B = 2, one u"""
    from oracle import unet_ddpm
    f = load_golden("hshift_ddpm.pt")
    cfg = unet_ddpm.DDPMConfig(**f["cfg"])
    from diffusion_pullback_amd import PullbackUNet
    net = PullbackUNet("ddpm", cfg, unet_ddpm.init_params(cfg, seed=f["seed"]), dtype=dtype, device=DEV, max_batch=2, max_rank=1, verbose=False)
    errs = {}
    for c in f["cases"]:
        e1 = net(f["x"], f["t"], u=c["u"], op=c["op"], block_idx=c["idx"])
        e2 = net(f["xb"], f["t"], u=c["u"], op=c["op"], block_idx=c["idx"])
        assert torch.is_tensor(e1) and e1.shape == c["eps"].shape and e2.shape == c["eps_b"].shape
        errs[(c["op"], c["idx"])] = (rel(e1, c["eps"]), rel(e2, c["eps_b"]))
    print(errs)
    assert all(max(v) < 2e-4 for v in errs.values()), errs
    c = f["cases"][0]                                                  # B rows of u: one per sample
    u2 = torch.cat([c["u"], torch.zeros_like(c["u"])])
    e2 = net(f["xb"], f["t"], u=u2, op="mid", block_idx=0).cpu()
    assert rel(e2[0:1], c["eps_b"][0:1]) < 2e-4 and torch.allclose(e2[1:2], net(f["xb"][1:2], f["t"]).cpu(), atol=1e-5, rtol=1e-4)
    with pytest.raises(ValueError):
        net(f["xb"], f["t"], u=c["u"], op="side", block_idx=0)
    with pytest.raises(ValueError):
        net(f["x"], f["t"], u=c["u"])                                  # a shift without its tap is not dropped


def test_forward_dh_and_h_traversal():
    S = _setup("sd")
    net = _net("sd", max_batch=3)
    e = net.engine
    x1, c1, t = S["x"][0:1], S["ctx"][0:1], S["t"]
    tap = ("mid", 0)
    u = S["u"][tap]
    shape = S["h"][tap][0].shape
    a = net.forward_dh(x1, t, c1, op="mid", block_idx=0, uk=u[0].reshape(shape))
    b = e.forward_shift(x1, float(t), c1, tap, u, [0], [1.0])
    assert torch.is_tensor(a) and torch.allclose(a, b, atol=1e-5, rtol=1e-4)
    a2 = net.forward_dh(S["x"], t, S["ctx"], op="up", block_idx=0, uk=S["u"][("up", 0)])       # one row of uk per sample
    b2 = e.forward_shift(S["x"], float(t), S["ctx"], ("up", 0), S["u"][("up", 0)], [0, 1], [1.0, 1.0])
    assert torch.allclose(a2, b2, atol=1e-5, rtol=1e-4)
    assert torch.allclose(net.forward_dh(x1, t, c1), net(x1, t, c1).sample, atol=1e-5, rtol=1e-4)
    with pytest.raises(TypeError, match="forward_dh"):
        net(x1, t, c1, uk=u[0], op="mid", block_idx=0)
    with pytest.raises(ValueError):
        net.forward_dh(x1, t, c1, op="mid", block_idx=1, uk=u[0])
    scales = [-1.5, 2.0]
    tr = net.h_traversal(x1, t, c1, u.T, scales, "mid", 0)              # 2 directions x 2 scales = 4 rows: calls of 3 + 1
    assert tr.shape == (2, 2, *x1.shape[1:])
    for i in range(2):
        for j, s in enumerate(scales):
            one = net.forward_dh(x1, t, c1, op="mid", block_idx=0, uk=(s * u[i] / u[i].norm()).reshape(shape))
            assert torch.allclose(tr[i, j], one[0], atol=1e-5, rtol=1e-4), (i, j)
    only = net.h_traversal(x1, t, c1, u.T, [2.0], "mid", 0, pcs=[1])
    assert torch.allclose(only[0, 0], tr[1, 1], atol=1e-5, rtol=1e-4)


def test_rejected_arguments_and_state_rules():
    from diffusion_pullback_amd import DpbError
    S = _setup("sd")
    net = _net("sd", max_batch=3)
    e = net.engine
    x1, c1, t = S["x"][0:1], S["ctx"][0:1], float(S["t"])
    tap = ("mid", 0)
    u = S["u"][tap]
    with pytest.raises(DpbError, match="batch=4 outside"):
        e.forward_shift(x1, t, c1, tap, u, [0] * 4, [1.0] * 4)
    with pytest.raises(DpbError, match="batch=0 outside"):
        e.forward_shift(x1, t, c1, tap, u, [], [])
    with pytest.raises(DpbError, match="xbatch=2"):
        e.forward_shift(S["x"], t, S["ctx"], tap, u, [0, 1, 0], [1.0] * 3)
    with pytest.raises(DpbError, match="nu=0"):
        e.forward_shift(x1, t, c1, tap, u[:0], [0], [1.0])
    for bad in ([0, 2], [-2, 0]):
        with pytest.raises(DpbError, match="outside"):
            e.forward_shift(x1, t, c1, tap, u, bad, [1.0, 1.0])
    with pytest.raises(DpbError, match="not downstream"):
        e.forward_shift(x1, t, c1, tap, u, [0], [1.0], dst=("down", 0))
    with pytest.raises(DpbError, match="not downstream"):
        e.forward_shift(x1, t, c1, "eps", torch.zeros(1, e.tap_numel("eps")), [0], [1.0], dst="eps")
    temb = e.tape.temb_in                                              # a buffer that does not depend on x is no tap to shift
    e.tape.taps["temb"] = temb; e.tape.tap_shape[temb] = (e.tape.buffers[temb][1], 1, 1)
    try:
        with pytest.raises(DpbError, match="invalid source buffer"):
            e.forward_shift(x1, t, c1, "temb", torch.zeros(1, e.tap_numel("temb")), [0], [1.0])
    finally:
        del e.tape.taps["temb"], e.tape.tap_shape[temb]
    e.primal(x1, t, c1, "eps")
    e.forward_shift(x1, t, c1, tap, u, [0, 1], [1.0, 1.0])
    with pytest.raises(DpbError):                                      # no stash was kept: a jvp right after the call is refused
        e.jvp_between(tap, "eps", torch.zeros(1, e.tap_numel(tap), device=DEV))
    with pytest.raises(DpbError):
        e.jvp(tap, torch.zeros(1, e.n_in, device=DEV))
    for kind in ("sd", "ddpm"):                                        # without shift arguments the call is the plain forward, bit for bit
        Sk = _setup(kind)
        nk = _net(kind, max_batch=2)
        xk, ck = Sk["x"], Sk["ctx"]
        a = nk(xk, Sk["t"], ck)
        a = a.sample if kind == "sd" else a
        assert torch.equal(a, nk.engine.forward(xk, float(Sk["t"]), ck, "eps"))
