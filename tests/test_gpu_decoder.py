"""GPU tests of the decoder pullback: the SVD of J_dec = d eps / d h at a tap, every skip connection held at its primal value
(PullbackUNet.local_decoder_pullback_xt / local_x0_decoder_pullback_xt / local_decoder_pullback_zt / get_h_to_e on the engine's
*_between entry points).

Yardsticks: the reference's own loops (tests/golden/make_golden_decoder.py: decoder_xt_ddpm.pt, decoder_zt_tiny.pt) and the fp32 CPU
restatement of get_h_to_e (tests/_decoder_ref.py).  Bars: golden singular vectors |cos| >= 0.9999 in fp32, >= 0.99 in 16 bit (there, for singular values within 5 % of each
other, the principal angles of their span), s within the encoder goldens' rtol 2e-3 (fp32); one direction of J v / J^T u within the per-dtype relative errors of
test_sd15_every_tap_one_direction_vs_oracle (fp32 5e-4, bf16 4e-2, fp16 1e-2)."""
import functools
import os

import pytest
import torch

from _decoder_ref import ddpm_h_to_e, sd_h_to_e
from _util import abs_cos, load_golden, oracle_jvp, oracle_vjp, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float32: 5e-4, torch.bfloat16: 4e-2, torch.float16: 1e-2}
COS = {torch.float32: 0.9999, torch.bfloat16: 0.99, torch.float16: 0.99}
S_RTOL = {torch.float32: 2e-3, torch.bfloat16: 4e-2, torch.float16: 2e-2}
T_SD = 696.2727


def _ddpm():
    from oracle import unet_ddpm
    f = load_golden("decoder_xt_ddpm.pt")
    cfg = unet_ddpm.DDPMConfig(**f["cfg"])
    return f, cfg, unet_ddpm.init_params(cfg, seed=f["seed"])


def _sd():
    from oracle import unet_sd
    f = load_golden("decoder_zt_tiny.pt")
    cfg = unet_sd.SDConfig(**f["cfg"])
    return f, cfg, unet_sd.init_params(cfg, seed=f["seed"], gain=f["gain"])


def _net(kind, cfg, p, dtype=torch.float32, max_batch=1, max_rank=4, upto=None):
    from diffusion_pullback_amd import PullbackUNet
    return PullbackUNet(kind, cfg, p, dtype=dtype, device=DEV, max_batch=max_batch, max_rank=max_rank, upto=upto, verbose=False)


def _clusters(s, gap=0.05):
    """index groups of singular values closer than `gap` (relative) to a neighbour"""
    out = [[0]]
    for i in range(1, len(s)):
        (out[-1].append(i) if s[i - 1] - s[i] < gap * s[i - 1] else out.append([i]))
    return out


def _cos_by_cluster(a, b, groups):
    """per-vector |cos| of rows; for a group of nearly equal singular values (16-bit only) the cosines of the principal angles between the
    spans: rounding of the order of the gap turns the vectors within such a span, which is all a per-vector bar would then measure"""
    out = []
    for g in groups:
        if len(g) == 1:
            out.append(abs_cos(a[g], b[g]))
        else:
            qa = torch.linalg.qr(a[g].double().T)[0]; qb = torch.linalg.qr(b[g].double().T)[0]
            out.append(torch.linalg.svdvals(qa.T @ qb))
    return torch.cat(out)


def _check(c, u, s, vT, dtype, scale=1.0):
    u, s, vT = u.cpu(), s.cpu(), vT.cpu()
    assert u.shape == c["u"].shape and vT.shape == c["vT"].shape
    assert torch.allclose(s, c["s"], rtol=S_RTOL[dtype]), (s, c["s"])
    groups = [[i] for i in range(len(s))] if dtype == torch.float32 else _clusters(c["s"].tolist())
    cu, cv = _cos_by_cluster(u.T, c["u"].T, groups), _cos_by_cluster(vT, c["vT"], groups)
    assert (cu > COS[dtype]).all() and (cv > COS[dtype]).all(), (groups, cu, cv)


# ------------------------------------------------------------------------------------------------ the reference's goldens
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", [0, 1])
def test_ddpm_decoder_xt_vs_reference(case, dtype):
    """PullBackDDPM.local_decoder_pullback_xt (diffusion.py:558-632): host-driven loop (same stop) and fused iterate (same count)"""
    f, cfg, p = _ddpm()
    c = f["xt"][case]
    net = _net("ddpm", cfg, p, dtype)
    u, s, vT = net.local_decoder_pullback_xt(f["x"], f["t"], op="mid", block_idx=0, pca_rank=c["k"], chunk_size=c["chunk_size"],
                                             min_iter=c["min_iter"], max_iter=c["max_iter"], convergence_threshold=c["thr"], V0=c["V0"])
    assert net.last_iters == c["iters"]
    _check(c, u, s, vT, dtype)
    u, s, vT, _ = net.decoder_pullback_fixed(f["x"], f["t"], None, "mid", 0, c["k"], c["iters"], c["V0"])
    _check(c, u, s, vT, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", [0, 1])
def test_ddpm_x0_decoder_xt_vs_reference(case, dtype):
    """PullBackDDPM.local_x0_decoder_pullback_xt (diffusion.py:634-710); the fused iterate rescaled by c = -sqrt(1 - a_t) / sqrt(a_t)"""
    f, cfg, p = _ddpm()
    c = f["x0"][case]
    net = _net("ddpm", cfg, p, dtype)
    u, s, vT = net.local_x0_decoder_pullback_xt(f["x"], f["t"], f["at"], op="mid", block_idx=0, pca_rank=c["k"], chunk_size=c["chunk_size"],
                                                min_iter=c["min_iter"], max_iter=c["max_iter"], convergence_threshold=c["thr"], V0=c["V0"])
    assert net.last_iters == c["iters"]
    _check(c, u, s, vT, dtype)
    cc = float(-(1 - f["at"]).sqrt() / f["at"].sqrt())
    u, s, vT, _ = net.decoder_pullback_fixed(f["x"], f["t"], None, "mid", 0, c["k"], c["iters"], c["V0"])
    _check(c, u, s * abs(cc), vT * cc, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", [0, 1, 2])
def test_sd_decoder_zt_vs_reference(case, dtype):
    """utils.local_decoder_pullback_zt (utils.py:818-898) on the toy SD net at 'mid', 'down' and 'up' taps"""
    f, cfg, p = _sd()
    c = f["cases"][case]
    net = _net("sd", cfg, p, dtype)
    u, s, vT = net.local_decoder_pullback_zt(f["z"], f["t"], f["ctx"], op=c["op"], block_idx=c["idx"], pca_rank=c["k"], chunk_size=c["chunk_size"],
                                             min_iter=c["min_iter"], max_iter=c["max_iter"], convergence_threshold=c["thr"], V0=c["V0"])
    assert net.last_iters == c["iters"]
    _check(c, u, s, vT, dtype)
    u, s, vT, _ = net.decoder_pullback_fixed(f["z"], f["t"], f["ctx"], c["op"], c["idx"], c["k"], c["iters"], c["V0"])
    _check(c, u, s, vT, dtype)


def test_zt_threshold_none_runs_max_iter():
    f, cfg, p = _sd()
    c = f["cases"][0]
    net = _net("sd", cfg, p)
    net.local_decoder_pullback_zt(f["z"], f["t"], f["ctx"], op="mid", block_idx=0, pca_rank=3, chunk_size=1, min_iter=0, max_iter=3, V0=c["V0"])
    assert net.last_iters == 3


# ------------------------------------------------------------------------------------------------ one direction vs the CPU restatement
def _threads():
    torch.set_num_threads(min(16, os.cpu_count() or 8))


@functools.lru_cache(maxsize=None)
def _sd15_setup(size):
    from diffusion_pullback_amd import configs as cf
    from oracle import unet_sd
    if size == "full":                 # the product's SD15 for the engine, the oracle's own SD15 for the restatement (seeded values shared)
        cfg, p = cf.SD15, cf.sd_init_params(cf.SD15, seed=0, spectrum=cf.Spectrum())
        taps = [("down", 1), ("mid", 0), ("up", 1)]
    else:   # medium: SD-1.5 layer widths and heads (head dim 40 / 80) at two levels on a 32 x 32 latent
        cfg = unet_sd.SDConfig(block_out_channels=(320, 640), layers_per_block=1, down_attn=(True, True), up_attn=(True, True), heads=(8, 8),
                               cross_dim=768, sample_size=32, ctx_len=77)
        p = unet_sd.init_params(cfg, seed=1)
        taps = [("down", 0), ("mid", 0), ("up", 0)]
    g = torch.Generator().manual_seed(3)
    s = cfg.sample_size
    z = torch.randn(1, 4, s, s, generator=g); ctx = torch.randn(1, 77, 768, generator=g)
    return cfg, p, z, ctx, taps


@functools.lru_cache(maxsize=None)
def _sd15_oracle(size):
    """h0, one direction V / J V and one cotangent U / J^T U of get_h_to_e per tap (fp32 CPU restatement, computed once)"""
    from oracle import unet_sd
    _threads()
    cfg, p, z, ctx, taps = _sd15_setup(size)
    cfg = unet_sd.SD15 if size == "full" else cfg
    t = torch.tensor(T_SD)
    g = torch.Generator().manual_seed(4)
    out = {}
    for tap in taps:
        with torch.no_grad():
            h0 = unet_sd.forward(p, cfg, z, t, ctx, stop=tap)
        fn = lambda h, tap=tap: sd_h_to_e(p, cfg, z, t, ctx, h, *tap)
        V = torch.randn(1, h0.numel(), generator=g)
        U = torch.randn(1, 4 * cfg.sample_size ** 2, generator=g)
        out[tap] = dict(V=V, JV=oracle_jvp(fn, h0, V), U=U, JTU=oracle_vjp(fn, h0, U))
    return out


def _one_direction(net, x, t, ctx, taps, oracle, dtype):
    e = net.engine
    e.primal(x, t, ctx, "eps")
    errs = {}
    for tap in taps:
        o = oracle[tap]
        JV = e.jvp_between(tap, "eps", o["V"].to(DEV)).cpu()
        JTU = e.vjp_between(tap, "eps", o["U"].to(DEV)).cpu()
        errs[tap] = (rel(JV, o["JV"]), rel(JTU, o["JTU"]))
        if dtype == torch.float32:            # adjointness <J v, u> = <v, J^T u>
            a, b = (JV.double() * o["U"].double()).sum(), (o["V"].double() * JTU.double()).sum()
            assert abs(a - b) <= 1e-5 * JV.double().norm() * o["U"].double().norm(), (tap, a, b)
    print(dtype, {k: tuple(round(x, 6) for x in v) for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not all(x < TOL[dtype] for x in v)}
    assert not bad, f"(jvp, vjp) relative errors over {TOL[dtype]}: {bad}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("size", ["medium", "full"])
def test_sd15_decoder_one_direction_vs_restatement(size, dtype):
    cfg, p, z, ctx, taps = _sd15_setup(size)
    net = _net("sd", cfg, p, dtype, max_rank=1)
    _one_direction(net, z, T_SD, ctx, taps, _sd15_oracle(size), dtype)


@functools.lru_cache(maxsize=None)
def _ddpm256():
    from diffusion_pullback_amd import configs as cf
    from oracle import unet_ddpm
    _threads()
    cfg = cf.CELEBA_HQ_256
    p = cf.ddpm_init_params(cfg, seed=0, spectrum=cf.Spectrum())
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 3, 256, 256, generator=g)
    t = torch.tensor(500.0)
    with torch.no_grad():
        h0 = unet_ddpm.forward(p, cfg, x, t, stop=("mid", 0))
    fn = lambda h: ddpm_h_to_e(p, cfg, x, t, h, "mid", 0)
    V = torch.randn(1, h0.numel(), generator=g); U = torch.randn(1, x.numel(), generator=g)
    return cfg, p, x, t, {("mid", 0): dict(V=V, JV=oracle_jvp(fn, h0, V), U=U, JTU=oracle_vjp(fn, h0, U))}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_ddpm256_decoder_one_direction_vs_restatement(dtype):
    cfg, p, x, t, oracle = _ddpm256()
    net = _net("ddpm", cfg, p, dtype, max_rank=1)
    _one_direction(net, x, float(t), None, [("mid", 0)], oracle, dtype)


# ------------------------------------------------------------------------------------------------ get_h_to_e
def test_get_h_to_e_forward_and_first_order():
    """get_h_to_e(h0) = eps of dpb_forward at every tap; at other h it is the CPU restatement; e(h0 + a d) - e(h0) = a J d to first order"""
    from oracle import unet_sd
    f, cfg, p = _sd()
    net = _net("sd", cfg, p, max_batch=3)
    z, t, ctx = f["z"], f["t"], f["ctx"]
    eps = net(z, t, ctx).sample.cpu()
    g = torch.Generator().manual_seed(6)
    for tap in [("down", 0), ("down", 1), ("mid", 0), ("up", 0)]:
        h0 = net.get_h(z, t, ctx, *tap).cpu()
        e0 = net.get_h_to_e(z, t, ctx, h0.repeat(2, 1, 1, 1), *tap).cpu()
        assert torch.allclose(e0, eps.expand(2, -1, -1, -1), atol=1e-5, rtol=1e-4), tap
        hr = h0 + 0.3 * torch.randn(3, *h0.shape[1:], generator=g)
        assert rel(net.get_h_to_e(sample=z, timestep=t, encoder_hidden_states=ctx, input_h=hr, op=tap[0], block_idx=tap[1]).cpu(),
                   sd_h_to_e(p, cfg, z, t, ctx, hr, *tap)) < 2e-4, tap
        d = torch.randn(1, *h0.shape[1:], generator=g)
        a = 1e-3
        de = net.get_h_to_e(z, t, ctx, h0 + a * d, *tap).cpu() - eps
        net.engine.primal(z, float(t), ctx, "eps")
        Jd = net.engine.jvp_between(tap, "eps", d.reshape(1, -1).to(DEV)).cpu().reshape(de.shape)
        assert rel(de, a * Jd) < 2e-2, (tap, rel(de, a * Jd))
    fd, cfgd, pd = _ddpm()
    netd = _net("ddpm", cfgd, pd)
    h0 = netd.get_h(fd["x"], fd["t"], op="mid", block_idx=0)
    assert torch.allclose(netd.get_h_to_e(fd["x"], fd["t"], h0, "mid", 0).cpu(), netd(fd["x"], fd["t"]).cpu(), atol=1e-5, rtol=1e-4)
    with pytest.raises(ValueError):
        net.get_h_to_e(z, t, ctx, torch.zeros(4, 64, 4, 4), "mid", 0)      # input_h.size(0) > max_batch


# ------------------------------------------------------------------------------------------------ fused iterate
def test_fused_decoder_iterate_equals_host_loop_and_batches():
    f, cfg, p = _sd()
    c = f["cases"][0]
    net = _net("sd", cfg, p, max_batch=2, max_rank=6)
    u, s, vT = net.local_decoder_pullback_zt(f["z"], f["t"], f["ctx"], op="mid", block_idx=0, pca_rank=3, chunk_size=3, min_iter=4, max_iter=4,
                                             convergence_threshold=None, V0=c["V0"])
    uf, sf, vTf, conv = net.decoder_pullback_fixed(f["z"], f["t"], f["ctx"], "mid", 0, 3, 4, c["V0"])
    assert torch.allclose(sf.cpu(), s.cpu(), rtol=1e-5) and torch.allclose(uf.cpu(), u.cpu(), atol=1e-5) and rel(vTf, vT) < 1e-5
    g = torch.Generator().manual_seed(7)
    zs = torch.cat([f["z"], torch.randn(1, 4, 8, 8, generator=g)]); ctxs = torch.cat([f["ctx"], torch.randn(1, 5, 16, generator=g)])
    ub, sb, vTb, _ = net.decoder_pullback_fixed(zs, f["t"], ctxs, "mid", 0, 3, 4, c["V0"])
    for i in range(2):
        ui, si, vTi, _ = net.decoder_pullback_fixed(zs[i:i + 1], f["t"], ctxs[i:i + 1], "mid", 0, 3, 4, c["V0"])
        assert torch.allclose(sb[3 * i:3 * i + 3].cpu(), si.cpu(), rtol=1e-4), (i, sb, si)
        assert (abs_cos(ub.T[3 * i:3 * i + 3], ui.T) > 0.9999).all() and (abs_cos(vTb[3 * i:3 * i + 3], vTi) > 0.9999).all()


def test_decoder_does_not_leak_into_encoder_path():
    """encoder iterate, decoder iterate, encoder iterate on ONE engine: the encoder results are bitwise equal, and equal to a fresh engine's"""
    f, cfg, p = _sd()
    V0e = torch.linalg.qr(torch.randn(256, 3, generator=torch.Generator().manual_seed(8)))[0].T.contiguous()
    for dtype in (torch.float32, torch.bfloat16):
        net = _net("sd", cfg, p, dtype)
        a = [t.cpu() for t in net.pullback_fixed(f["z"], f["t"], f["ctx"], "up", 0, 3, 3, V0e)]
        net.decoder_pullback_fixed(f["z"], f["t"], f["ctx"], "mid", 0, 3, 3, f["cases"][0]["V0"])
        net.local_decoder_pullback_zt(f["z"], f["t"], f["ctx"], op="down", block_idx=0, pca_rank=2, chunk_size=2, min_iter=0, max_iter=2,
                                      V0=f["cases"][1]["V0"][:2])
        b = [t.cpu() for t in net.pullback_fixed(f["z"], f["t"], f["ctx"], "up", 0, 3, 3, V0e)]
        fresh = [t.cpu() for t in _net("sd", cfg, p, dtype).pullback_fixed(f["z"], f["t"], f["ctx"], "up", 0, 3, 3, V0e)]
        for x, y, z in zip(a, b, fresh):
            assert torch.equal(x, y) and torch.equal(x, z), dtype


# ------------------------------------------------------------------------------------------------ error paths
def test_decoder_error_paths():
    from diffusion_pullback_amd import DpbError
    f, cfg, p = _sd()
    net = _net("sd", cfg, p)
    e = net.engine
    z, t, ctx = f["z"], f["t"], f["ctx"]
    e.primal(z, float(t), ctx, "eps")
    with pytest.raises(DpbError, match="not downstream"):
        e.jvp_between(("mid", 0), ("down", 0), torch.zeros(1, 1024, device=DEV))
    with pytest.raises(DpbError, match="scratch"):
        e.iterate_between(("mid", 0), "eps", torch.zeros(3, 1024, device=DEV), 1, scratch=torch.empty(1024, dtype=torch.uint8, device=DEV))
    e.primal(z, float(t), ctx, ("mid", 0))                # a primal that stops before eps
    with pytest.raises(DpbError, match="no primal state"):
        e.jvp_between(("mid", 0), "eps", torch.zeros(1, 1024, device=DEV))
    e.forward(z, float(t), ctx)                           # forward keeps no state
    with pytest.raises(DpbError):
        e.vjp_between(("mid", 0), "eps", torch.zeros(1, 256, device=DEV))
    with pytest.raises(ValueError, match="batch 1"):
        net.local_decoder_pullback_zt(z.repeat(2, 1, 1, 1), t, ctx, op="mid", block_idx=0, pca_rank=2, chunk_size=2, max_iter=1)
    short = _net("sd", cfg, p, upto=("mid", 0))
    with pytest.raises(ValueError, match="up to eps"):
        short.local_decoder_pullback_zt(z, t, ctx, op="mid", block_idx=0, pca_rank=2, chunk_size=2, max_iter=1)
    with pytest.raises(ValueError, match="up to eps"):
        short.get_h_to_e(z, t, ctx, torch.zeros(1, 64, 4, 4), "mid", 0)


def test_passes_leave_nothing_behind_for_the_next_pass():
    """A pass with another seed, or a call refused in validation, leaves nothing behind that a later pass reads: jvp_between, jvp, (a refused
    forward_from), vjp_between -- then the same three passes again, bit for bit."""
    from diffusion_pullback_amd import DpbError
    f, cfg, p = _sd()
    e = _net("sd", cfg, p, torch.bfloat16, max_rank=2).engine
    z, t, ctx = f["z"], float(f["t"]), f["ctx"]
    mid = ("mid", 0)
    g = torch.Generator().manual_seed(11)
    V = torch.randn(2, e.tap_numel(mid), generator=g).to(DEV)
    Vx = torch.randn(2, e.n_in, generator=g).to(DEV)
    e.primal(z, t, ctx, "eps")
    U1 = e.jvp_between(mid, "eps", V)
    A1 = e.jvp(mid, Vx)
    with pytest.raises(DpbError, match="not downstream"):
        e.forward_from(z, t, ctx, mid, torch.zeros(1, e.tap_numel(mid)), dst=("down", 0))
    W1 = e.vjp_between(mid, "eps", U1)
    U2 = e.jvp_between(mid, "eps", V)
    A2 = e.jvp(mid, Vx)
    W2 = e.vjp_between(mid, "eps", U1)
    assert torch.equal(U1, U2) and torch.equal(A1, A2) and torch.equal(W1, W2)
    assert U1.abs().max() > 0 and A1.abs().max() > 0 and W1.abs().max() > 0
