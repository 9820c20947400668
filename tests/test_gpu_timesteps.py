"""Per-sample timesteps (dpb_primal_t / dpb_forward_t): row b of a batch run at t = [t_0, .., t_{B-1}] is the net at (x_b, t_b, ctx_b).

The bar of the row-identity tests is bitwise equality with the SAME batch run at the scalar t_b: same batch means same tiles, the engine is bitwise
reproducible by default, and a sample's row of the time-embedding path is computed by the launches of a scalar call.  Every test here runs toy
nets (the toy SD / DDPM of tests/test_gpu_parity.py at latent sides 8, 12 and 16)."""
import csv

import pytest
import torch

from _util import abs_cos, load_golden

pytestmark = pytest.mark.gpu

TS = [696.2727, 301.0, 17.5]


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return "cuda:0"


def _net(kind, side, dtype, max_batch=3, max_rank=9, boc=(32, 64)):
    """the toy nets of test_gpu_parity.py at latent side `side`: SD levels side, side / 2; DDPM levels side, side / 2, side / 4"""
    from diffusion_pullback_amd import PullbackUNet
    g = torch.Generator().manual_seed(5)
    if kind == "sd":
        from oracle import unet_sd
        f = load_golden("pullback_zt_tiny.pt")
        cfg = unet_sd.SDConfig(**{**f["cfg"], "sample_size": side, "block_out_channels": boc})
        p = unet_sd.init_params(cfg, seed=f["seed"], gain=f["gain"])
        x, ctx = torch.randn(3, 4, side, side, generator=g), torch.randn(3, 5, 16, generator=g)
    else:
        from oracle import unet_ddpm
        f = load_golden("ddpm_small.pt")
        cfg = unet_ddpm.DDPMConfig(**{**f["cfg"], "resolution": side, "attn_resolutions": (side // 2,)})
        p = unet_ddpm.init_params(cfg, seed=f["seed"])
        x, ctx = torch.randn(3, 3, side, side, generator=g), None
    return PullbackUNet(kind, cfg, p, dtype=dtype, device=_dev(), max_batch=max_batch, max_rank=max_rank, verbose=False), x, ctx


def _eps(net, x, t, ctx):
    return net(x, t, ctx).sample if net.kind == "sd" else net(x, t)


def _features(net, x, t, ctx):
    """get_h at every tap, and eps, through the public surface"""
    out = {}
    for key in net.engine.tape.taps:
        if key == "eps":
            out[key] = _eps(net, x, t, ctx)
        elif net.kind == "sd":
            out[key] = net.get_h(x, t, ctx, op=key[0], block_idx=key[1])
        else:
            out[key] = net.get_h(x=x, t=t, op=key[0], block_idx=key[1])
    return out


def _assert_rows_are_the_scalar_runs(net, x, ctx, what):
    het = _features(net, x, torch.tensor(TS), ctx)
    refs = [_features(net, x, TS[i], ctx) for i in range(3)]
    for key, h in het.items():
        assert torch.isfinite(h).all(), (what, key)
        for i in range(3):
            assert torch.equal(h[i], refs[i][key][i]), f"{what} tap {key} row {i}: max |d| = {(h[i] - refs[i][key][i]).abs().max().item():.3e}"
    # the timesteps do matter: the same row at another sample's timestep is another tensor (the identity above is not vacuous)
    assert not torch.equal(refs[0]["eps"][1], refs[1]["eps"][1]) and not torch.equal(refs[2]["eps"][1], refs[1]["eps"][1])


@pytest.mark.parametrize("side", [16, 8, 12])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", ["sd", "ddpm"])
def test_each_row_of_a_mixed_timestep_batch_is_bitwise_the_scalar_run(kind, dtype, side):
    """x [3] at t = [a, b, c] with per-sample ctx: row i of get_h at every tap and of eps equals row i of the same batch at the scalar t_i, bit
    for bit; again with x repeated (fix_xt: the rows differ in t only).  Side 8 (SD levels 8, 4: 64 and 16 rows per sample; DDPM 8, 4, 2) puts
    several samples into one 64-row tile, so one tile reads several bias rows; side 12 gives 144 / 36 (/ 9) rows, a multiple of no tile."""
    net, x, ctx = _net(kind, side, dtype)
    _assert_rows_are_the_scalar_runs(net, x, ctx, "distinct x")
    _assert_rows_are_the_scalar_runs(net, x[:1].repeat(3, 1, 1, 1), ctx, "fix_xt")


def _tile_codes():
    from test_gpu_gemm_tiles import KIND_16BIT                      # the forced codes that test lists: the 16-bit table, 128 (fp32) and 600 (halo)
    return sorted(KIND_16BIT) + [128, 600]


# dpb_debug_set has no getter.  Both switches start at 0 (the heuristic: gemm.hip's g_force_tile / g_force_splitk, with no environment override) and every
# test that forces them puts 0 back, so 0 IS the previous value that `finally` restores.
def _restore_switches(lib, L):
    L.check(lib.dpb_debug_set(b"gemm_tile", 0))
    L.check(lib.dpb_debug_set(b"gemm_splitk", 0))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_row_identity_holds_under_every_forced_tile_and_split(dtype):
    """The same identity (eps, 64- and 128-channel toy SD so that the 64-channel conv tiles take its ResBlock products) with every tile code
    forced, and with gemm_splitk forced to 1 and to 3.  The fp32 engine has two tiles (64, 128: it never leaves the register-staged kernel)."""
    from diffusion_pullback_amd import lib as L
    lib = L.load()
    net, x, ctx = _net("sd", 8, dtype, boc=(64, 128))
    tt = torch.tensor(TS)
    try:
        for key, values in (("gemm_tile", _tile_codes() if dtype != torch.float32 else [64, 128]), ("gemm_splitk", [1, 3])):
            for v in values:
                L.check(lib.dpb_debug_set(key.encode(), v))
                het = _eps(net, x, tt, ctx)
                assert torch.isfinite(het).all(), (key, v)
                for i in range(3):
                    ref = _eps(net, x, TS[i], ctx)
                    assert torch.equal(het[i], ref[i]), f"{key}={v} row {i}: max |d| = {(het[i] - ref[i]).abs().max().item():.3e}"
            L.check(lib.dpb_debug_set(key.encode(), 0))
    finally:
        _restore_switches(lib, L)


def _rowbias_engine(H, cin, cout, ks, dtype, g, col=16):
    """ONE row-bias product: temb [1][8] -> Linear -> proj [1][col + round8(cout)] (SHARED), then a ks x ks convolution of x [H*H][cin] whose
    row bias is the window [col, col + cout) of proj -- the bias buffer's pitch is not the product's N, and the window does not start at 0"""
    from diffusion_pullback_amd import lib as L
    from diffusion_pullback_amd.engine import Engine
    from diffusion_pullback_amd.tape import Tape
    width = col + (cout + 7) // 8 * 8
    p = {"c.weight": torch.randn(cout, cin, ks, ks, generator=g) * 0.05, "c.bias": torch.randn(cout, generator=g),
         "tp.weight": torch.randn(width, 8, generator=g), "tp.bias": torch.randn(width, generator=g)}
    t = Tape(p, dtype, torch.device(_dev()))
    t.temb_in = t.buf(1, 8, L.BUF_SHARED)
    t.x = t.buf(H * H, cin)
    proj = t.conv("tp", t.temb_in, (1, 1), width, ks=1, need_adj=False, kind=L.BUF_SHARED)
    o = t.conv("c", t.x, (H, H), cout, ks=ks, stride=1, pad=ks // 2, rowbias=proj, rowbias_off=col)
    t.tap("o", o, cout, H, H)
    return Engine(t, 8, False, True, cin, max_batch=3, max_tangents=3), torch.randn(3, cin, H, H, generator=g).cuda()


def _rowbias_run(e, x, t, path=None):
    """the product's output; with `path`: profiling on, and the profile kind (`big` column of the dump) of the LAST launch, the row-bias product"""
    if path is None:
        e.primal(x, t, None, "o")
        return e.read("o").clone(), e.stats()[0]
    e.profile(True)
    e.primal(x, t, None, "o")
    out = e.read("o").clone()
    e.profile_dump(str(path))
    e.profile(False)
    with open(path) as fh:
        kinds = [int(r["big"]) for r in csv.DictReader(fh)]
    return out, kinds[-1]


def _assert_rowbias_rows(e, x, what, path=None):
    het, extra = _rowbias_run(e, x, TS, path)
    assert torch.isfinite(het).all(), what
    refs = [_rowbias_run(e, x, TS[i])[0] for i in range(3)]
    for i in range(3):
        assert torch.equal(het[i], refs[i][i]), f"{what} row {i}: max |d| = {(het[i] - refs[i][i]).abs().max().item():.3e}"
    assert not torch.equal(refs[0][1], refs[1][1]), what              # the bias row does matter
    return extra


def test_every_forced_tile_takes_the_row_bias_product_itself(tmp_path):
    """Op level, as tests/test_gpu_gemm_tiles.py: ONE row-bias product per engine, batch 3 at 64 rows per sample (every tile but the 64-row ones
    spans samples), bias window at column 16 of a wider buffer.  Under each forced code the product's launch is bracketed with the profile kind of
    THAT code's tile (include/dpb.h; the weights-resident kernel takes no row operand of this kind: its documented substitute 515, kind 4) -- no
    silent substitute -- and each row equals the same batch at that row's scalar t, bit for bit."""
    from diffusion_pullback_amd import lib as L
    from test_gpu_gemm_tiles import KIND_16BIT
    lib = L.load()
    g = torch.Generator().manual_seed(17)
    wrong = {}
    try:
        e, x = _rowbias_engine(8, 320, 320, 1, torch.bfloat16, g)
        for code, kind in sorted(KIND_16BIT.items()):
            L.check(lib.dpb_debug_set(b"gemm_tile", code))
            got = _assert_rowbias_rows(e, x, f"bf16 1x1 code {code}", tmp_path / "p.csv")
            if got != (4 if code == 540 else kind):
                wrong[code] = got
        del e
        e, x = _rowbias_engine(8, 64, 128, 3, torch.bfloat16, g)          # 3x3: the halo-tile kernel's epilogue
        for code, kind in ((515, 4), (600, 5)):
            L.check(lib.dpb_debug_set(b"gemm_tile", code))
            got = _assert_rowbias_rows(e, x, f"bf16 3x3 code {code}", tmp_path / "p.csv")
            if got != kind:
                wrong[("3x3", code)] = got
        del e
        e, x = _rowbias_engine(8, 320, 320, 1, torch.float32, g)
        for code, kind in ((64, 0), (128, 1)):
            L.check(lib.dpb_debug_set(b"gemm_tile", code))
            got = _assert_rowbias_rows(e, x, f"fp32 code {code}", tmp_path / "p.csv")
            if got != kind:
                wrong[("fp32", code)] = got
        assert not wrong, f"forced code -> profile kind of the row-bias product, where it is not the code's own: {wrong}"
    finally:
        _restore_switches(lib, L)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("cout", [320, 100])
def test_split_k_reduction_and_scalar_tails_take_the_sample_bias_row(dtype, cout):
    """gemm_splitk forced to 3 sends the row-bias product through splitk_reduce_kernel (one launch more than unsplit).  cout = 100 is no multiple
    of 8: the non-vector branch of the reduction and the scalar tails of the epilogues form the per-sample address (register-staged tile 64, and
    in 16 bit the ring tile 515)."""
    from diffusion_pullback_amd import lib as L
    lib = L.load()
    g = torch.Generator().manual_seed(19)
    e, x = _rowbias_engine(8, 320, cout, 1, dtype, g)                        # K = 320: five 64-deep chunks to split
    try:
        for code in ([0, 64] if dtype == torch.float32 else [0, 64, 515]):
            L.check(lib.dpb_debug_set(b"gemm_tile", code))
            n = {}
            for split in (1, 3):
                L.check(lib.dpb_debug_set(b"gemm_splitk", split))
                _assert_rowbias_rows(e, x, f"{dtype} cout {cout} code {code} splitk {split}")
                n[split] = _rowbias_run(e, x, TS[0])[1]
            assert n[3] > n[1], (code, n)                                    # the reduction ran
    finally:
        _restore_switches(lib, L)


@pytest.mark.parametrize("kind", ["sd", "ddpm"])
def test_equal_timesteps_are_the_scalar_call(kind):
    """t = [a, a, a] is the scalar entry point: same bits, same number of launches (dpb_engine_stats)"""
    net, x, ctx = _net(kind, 8, torch.bfloat16)
    a = _eps(net, x, TS[0], ctx)
    n_a = net.engine.stats()[0]
    b = _eps(net, x, torch.tensor([TS[0]] * 3), ctx)
    n_b = net.engine.stats()[0]
    c = _eps(net, x, torch.tensor(TS), ctx)
    n_c = net.engine.stats()[0]
    assert torch.equal(a, b) and n_a == n_b, (n_a, n_b)
    assert n_c > n_a and not torch.equal(a, c)                       # distinct timesteps: the time-embedding chain once per sample
    net.engine.primal(x, TS[0], ctx, "eps")
    n_p = net.engine.stats()[0]
    net.engine.primal(x, [TS[0]] * 3, ctx, "eps")
    assert net.engine.stats()[0] == n_p


def _close(s_a, s_b, rows_a, rows_b, what):
    """the bar of test_batched_samples_match_single_sample_runs (fp32): s rtol 1e-4, |cos| > 0.9999"""
    assert torch.allclose(s_a, s_b, rtol=1e-4), (what, s_a, s_b)
    cos = abs_cos(rows_a, rows_b)
    assert (cos > 0.9999).all(), (what, cos)


def test_passes_on_a_mixed_timestep_primal_match_single_sample_runs():
    """jvp, vjp and pullback_fixed after a primal at t = [a, b, c]: per sample what the single-sample run at that sample's t gives"""
    net, x, ctx = _net("sd", 8, torch.float32)
    g = torch.Generator().manual_seed(7)
    key, k = ("mid", 0), 3
    V = torch.randn(3 * k, net.engine.n_in, generator=g).cuda()
    Uc = torch.randn(3 * k, net.engine.tap_numel(key), generator=g).cuda()
    net.engine.primal(x, torch.tensor(TS), ctx, key)
    J, Jt = net.engine.jvp(key, V).clone(), net.engine.vjp(key, Uc).clone()
    V0 = torch.linalg.qr(torch.randn(net.engine.n_in, k, generator=g))[0].T.contiguous()
    _, s_b, V_b, _ = net.pullback_fixed(x, torch.tensor(TS), ctx, "mid", 0, k, 4, V0)
    for i in range(3):
        r = slice(k * i, k * i + k)
        net.engine.primal(x[i:i + 1], TS[i], ctx[i:i + 1], key)
        J_i, Jt_i = net.engine.jvp(key, V[r]), net.engine.vjp(key, Uc[r])
        _close(J[r].norm(dim=1), J_i.norm(dim=1), J[r], J_i, f"jvp {i}")
        _close(Jt[r].norm(dim=1), Jt_i.norm(dim=1), Jt[r], Jt_i, f"vjp {i}")
        _, s_i, V_i, _ = net.pullback_fixed(x[i:i + 1], TS[i], ctx[i:i + 1], "mid", 0, k, 4, V0)
        _close(s_b[r], s_i, V_b[r], V_i, f"pullback_fixed {i}")
        if i:                                                       # ... and not what sample i gives at sample 0's timestep
            _, s_0, _, _ = net.pullback_fixed(x[i:i + 1], TS[0], ctx[i:i + 1], "mid", 0, k, 4, V0)
            assert not torch.allclose(s_b[r], s_0, rtol=1e-4)


def test_decoder_pullback_fixed_and_global_pca_honour_per_sample_timesteps():
    """decoder_pullback_fixed after a primal at t = [a, b, c]: per sample the single-sample run at that t (bar of _close).  global_pca_zt with a
    timestep per sample, in chunks of 4 + 2 (the timesteps sliced with the chunks), against the same call one sample at a time -- every sample
    through the scalar entry point at its own t; same seed, so the same R."""
    net, x, ctx = _net("sd", 8, torch.float32, max_batch=4)
    g = torch.Generator().manual_seed(23)
    k, n_h = 2, net.engine.tap_numel(("mid", 0))
    V0 = torch.linalg.qr(torch.randn(n_h, k, generator=g))[0].T.contiguous()
    _, s_b, U_b, _ = net.decoder_pullback_fixed(x, torch.tensor(TS), ctx, "mid", 0, k, 4, V0)
    for i in range(3):
        r = slice(k * i, k * i + k)
        _, s_i, U_i, _ = net.decoder_pullback_fixed(x[i:i + 1], TS[i], ctx[i:i + 1], "mid", 0, k, 4, V0)
        _close(s_b[r], s_i, U_b[r], U_i, f"decoder_pullback_fixed {i}")
    _, s_0, _, _ = net.decoder_pullback_fixed(x[1:2], TS[0], ctx[1:2], "mid", 0, k, 4, V0)
    assert not torch.allclose(s_b[k:2 * k], s_0, rtol=1e-4)                  # ... and not sample 1 at sample 0's timestep
    xs = torch.randn(6, 4, 8, 8, generator=g)
    ts = torch.tensor(TS + [850.0, 520.25, 99.0])
    out = []
    for mb in (4, 1):
        torch.manual_seed(29)
        out.append(net.global_pca_zt(xs, ts, ctx[:1], op="mid", block_idx=0, memory_bound=mb, pca_rank=3))
    (u4, s4), (u1, s1) = out
    _close(s4, s1, u4.T, u1.T, "global_pca_zt")
    torch.manual_seed(29)
    _, s_shared = net.global_pca_zt(xs, ts[0], ctx[:1], op="mid", block_idx=0, memory_bound=4, pca_rank=3)
    assert not torch.allclose(s4, s_shared, rtol=1e-4)
    with pytest.raises(ValueError, match="elements for a batch"):
        net.global_pca_zt(xs, ts[:4], ctx[:1], op="mid", block_idx=0, memory_bound=4, pca_rank=3)


@pytest.mark.parametrize("kind", ["sd", "ddpm"])
def test_batch_pullback_stops_each_sample_by_its_own_rule_and_freezes_it(kind):
    """Thresholds [inf, 0, inf] with min_iter 2, max_iter 6: samples 0 and 2 stop at the first i > min_iter (i = 3: 4 iterations, as _pullback
    counts them), sample 1 runs out max_iter.  Each sample matches the single-sample method at its (x, t, ctx, threshold); the snapshot of
    sample 0 does not move when the others iterate on (max_iter 9)."""
    net, x, ctx = _net(kind, 8, torch.float32, max_rank=6)
    k, thr = 2, [float("inf"), 0.0, float("inf")]
    g = torch.Generator().manual_seed(3)
    V0 = torch.linalg.qr(torch.randn(net.engine.n_in, k, generator=g))[0].T.contiguous()
    kw = dict(op="mid", block_idx=0, pca_rank=k, min_iter=2)
    u, s, vT, iters = net.local_encoder_pullback_batch(x, torch.tensor(TS), ctx, max_iter=6, convergence_threshold=thr, V0=V0, **kw)
    assert iters.tolist() == [4, 6, 4], iters
    n_h = net.engine.tap_numel(("mid", 0))
    assert tuple(u.shape) == (3, n_h, k) and tuple(s.shape) == (3, k) and tuple(vT.shape) == (3, k, net.engine.n_in)
    for b in range(3):
        if kind == "sd":
            u1, s1, v1 = net.local_encoder_pullback_zt(x[b:b + 1], TS[b], ctx[b:b + 1], max_iter=6, convergence_threshold=thr[b], V0=V0, chunk_size=k, **kw)
        else:
            u1, s1, v1 = net.local_encoder_pullback_xt(x[b:b + 1], TS[b], max_iter=6, convergence_threshold=thr[b], V0=V0, chunk_size=k, **kw)
        assert net.last_iters == iters[b]
        _close(s[b], s1, vT[b], v1, f"sample {b} vT")
        _close(s[b], s1, u[b].T, u1.T, f"sample {b} u")
    u9, s9, vT9, iters9 = net.local_encoder_pullback_batch(x, torch.tensor(TS), ctx, max_iter=9, convergence_threshold=thr, V0=V0, **kw)
    assert iters9.tolist() == [4, 9, 4], iters9
    for b in (0, 2):
        assert torch.equal(u9[b], u[b]) and torch.equal(s9[b], s[b]) and torch.equal(vT9[b], vT[b]), b
    with pytest.raises(ValueError, match="max_rank"):
        net.local_encoder_pullback_batch(x, torch.tensor(TS), ctx, max_iter=6, op="mid", block_idx=0, pca_rank=3)
    with pytest.raises(ValueError, match="max_batch"):
        net.local_encoder_pullback_batch(x.repeat(2, 1, 1, 1), TS[0], None if ctx is None else ctx.repeat(2, 1, 1), max_iter=6, op="mid", block_idx=0, pca_rank=1)


def test_refusals():
    """A timestep tensor of a length that is neither 1 nor B, and distinct timesteps where a call takes one for its batch, raise ValueError;
    dpb_primal_t with distinct timesteps on an autoencoder tape (nothing reads its timestep slot) fails with a message."""
    from diffusion_pullback_amd import DpbError, configs as cf
    from diffusion_pullback_amd.vae import AutoencoderKL
    net, x, ctx = _net("sd", 8, torch.float32)
    tt = torch.tensor(TS)
    with pytest.raises(ValueError, match="elements for a batch"):
        net.get_h(x, torch.tensor(TS[:2]), ctx, op="mid", block_idx=0)
    with pytest.raises(ValueError, match="elements for a batch"):
        net(x[:2], tt, ctx[:2])
    n_h = net.engine.tap_numel(("mid", 0))
    with pytest.raises(ValueError, match="one timestep"):
        net.forward_dh(x, tt, ctx, op="mid", block_idx=0, uk=torch.zeros(1, n_h))
    with pytest.raises(ValueError, match="one timestep"):
        net.get_h_to_e(x[:1], tt, ctx[:1], torch.zeros(3, n_h), op="mid", block_idx=0)
    with pytest.raises(ValueError, match="one timestep"):
        net.local_pca_zt(x[:1], tt, ctx[:1], op="mid", block_idx=0, num_pca_samples=6, memory_bound=3, pca_rank=2)
    e = net.forward_dh(x, torch.tensor([TS[1]] * 3), ctx, op="mid", block_idx=0, uk=torch.zeros(1, n_h))     # equal timesteps are one timestep
    assert torch.equal(e, _eps(net, x, TS[1], ctx))
    vcfg = cf.VAEConfig(block_out_channels=(32, 64, 64), layers_per_block=1, groups=8, sample_size=32)
    vae = AutoencoderKL(vcfg, cf.vae_init_params(vcfg, seed=1), dtype=torch.bfloat16, device=_dev(), max_batch=2, encoder=False)
    z = torch.randn(2, vcfg.latent_channels, vcfg.latent_size, vcfg.latent_size)
    vae.dec.primal(z, [0.0, 0.0], None, "image")                    # equal: the scalar call
    with pytest.raises(DpbError, match="without a timestep embedding"):
        vae.dec.primal(z, [0.0, 1.0], None, "image")
