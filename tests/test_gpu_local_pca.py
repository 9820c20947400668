"""GPU tests of local h-space PCA: the noise kernel (dpb_perturb_unit) with injected and with generated noise, the sampling loop
(dpb_local_pca_sample), and the bind()-attached local_pca_zt / local_pca_xt / global_pca_xt / inv_jac_xt against the reference's goldens
(tests/golden/make_golden_local_pca.py), reproducibility, error paths and isolation from the pullback."""
import pytest
import torch

from _local_pca_ref import philox_normals, position_at_R, reference_pairing
from _util import abs_cos, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x9E3779B97F4A7C15          # both key words in use


class _Unet:
    """stands in for the diffusers module bind() patches: only state_dict() is read"""

    def __init__(self, p):
        self._p = p

    def state_dict(self):
        return self._p


def _sd(dtype=torch.float32, max_batch=5, max_rank=4):
    from diffusion_pullback_amd import bind
    from oracle import unet_sd
    g = load_golden("local_pca_zt_tiny.pt")
    cfg = unet_sd.SDConfig(**g["cfg"])
    unet = _Unet(unet_sd.init_params(cfg, seed=g["seed"], gain=g["gain"]))
    impl = bind(unet, "sd", cfg, dtype=dtype, device=DEV, max_batch=max_batch, max_rank=max_rank, verbose=False)
    return g, unet, impl


def _ddpm(dtype=torch.float32, max_batch=5, max_rank=4):
    from diffusion_pullback_amd import bind
    from oracle import unet_ddpm
    g = load_golden("local_pca_xt_ddpm.pt")
    cfg = unet_ddpm.DDPMConfig(**g["cfg"])
    unet = _Unet(unet_ddpm.init_params(cfg, seed=g["seed"]))
    impl = bind(unet, "ddpm", cfg, dtype=dtype, device=DEV, max_batch=max_batch, max_rank=max_rank, verbose=False)
    return g, unet, impl


def _ulp(v):
    """fp32 spacing at magnitude v (a positive python float)"""
    return float(torch.nextafter(torch.tensor(v, dtype=torch.float32), torch.tensor(float("inf"))) - torch.tensor(v, dtype=torch.float32))


# ------------------------------------------------------------------ the kernel with injected noise
@pytest.mark.parametrize("n", [1, 3, 1023, 4100, 16384, 196608])       # ragged (no 16-byte path), below / across the 4096-element slice, SD and DDPM-256 sizes
@pytest.mark.parametrize("B", [1, 5, 7])
def test_perturb_unit_injected_noise_against_fp64(n, B):
    from diffusion_pullback_amd.engine import perturb_unit
    gen = torch.Generator().manual_seed(1000 * B + n % 997)
    x = torch.randn(n, generator=gen).to(DEV)
    noise = torch.randn(B, n, generator=gen).to(DEV)
    for norm in (1.0, 2.5):
        out, g = perturb_unit(x, B, noise=noise, norm=norm, return_noise=True)
        assert torch.equal(g, noise)
        ref = x.double() + norm * noise.double() / noise.double().norm(dim=1, keepdim=True)
        got = (out.double() - x.double()).norm(dim=1)
        assert ((got - norm).abs() / norm).max().item() <= 1e-6, (n, B, norm, got.tolist())
        # 2 ulp at the magnitude of the data: the result is rounded once at its own magnitude (<= 1/2 ulp) and the factor norm / ||g|| once
        # (relative 2^-24 of a perturbation no larger than |x| + |out|)
        tol = 2 * _ulp(max(x.abs().max().item(), ref.abs().max().item()))
        assert (out.double() - ref).abs().max().item() <= tol, (n, B, norm, (out.double() - ref).abs().max().item(), tol)


# ------------------------------------------------------------------ generated mode
def test_generated_noise_is_the_documented_philox_box_muller():
    from diffusion_pullback_amd.engine import perturb_unit
    n, B, first = 4100, 3, 2 ** 40 + 5
    x = torch.randn(n, generator=torch.Generator().manual_seed(3)).to(DEV)
    out, g = perturb_unit(x, B, seed=SEED, first=first, return_noise=True)
    want = torch.stack([philox_normals(SEED, first + b, n) for b in range(B)])
    err = (g.double().cpu() - want).abs().max().item()
    assert err <= 1e-5, err                                  # a wrong constant, word order or counter layout misses by O(1)
    ref = x.double().cpu() + want / want.norm(dim=1, keepdim=True)
    assert (out.double().cpu() - ref).abs().max().item() <= 1e-6
    # the low and the high word of seed and sample index both matter
    for s2, f2 in ((SEED ^ (1 << 32), first), (SEED ^ 1, first), (SEED, first ^ (1 << 40)), (SEED, first + 1)):
        _, g2 = perturb_unit(x, 1, seed=s2, first=f2, return_noise=True)
        assert (g2[0] - g[0]).abs().max().item() > 1.0


@pytest.mark.parametrize("n", [4100, 1023])
def test_generated_sample_is_independent_of_batch_and_first(n):
    from diffusion_pullback_amd.engine import perturb_unit
    x = torch.randn(n, generator=torch.Generator().manual_seed(4)).to(DEV)
    out7, g7 = perturb_unit(x, 7, seed=SEED, first=0, return_noise=True)
    for i in range(7):
        o1, g1 = perturb_unit(x, 1, seed=SEED, first=i, return_noise=True)
        assert torch.equal(o1[0], out7[i]) and torch.equal(g1[0], g7[i]), i
    o3 = perturb_unit(x, 3, seed=SEED, first=2)
    assert torch.equal(o3, out7[2:5])
    again, g_again = perturb_unit(x, 7, seed=SEED, first=0, return_noise=True)
    assert torch.equal(again, out7) and torch.equal(g_again, g7)
    assert torch.equal(perturb_unit(x, 7, seed=SEED, first=0), out7)       # with and without noise_out


def test_generated_noise_statistics():
    from diffusion_pullback_amd.engine import perturb_unit
    x = torch.zeros(2 ** 18, device=DEV)
    _, g = perturb_unit(x, 4, seed=11, first=0, return_noise=True)          # 2^20 values: 5 sigma of the mean is 5 / 1024, of the variance 5 sqrt(2) / 1024
    assert g.double().mean().abs().item() <= 0.005 and abs(g.double().var().item() - 1) <= 0.01
    n = 196608                                                              # |cos| of independent rows ~ N(0, 1/n): 5 sigma = 0.0113
    x = torch.zeros(n, device=DEV)
    _, a = perturb_unit(x, 2, seed=0, first=0, return_noise=True)
    _, b = perturb_unit(x, 1, seed=1, first=0, return_noise=True)
    assert abs_cos(a[0:1], a[1:2]).item() <= 0.012 and abs_cos(a[0:1], b[0:1]).item() <= 0.012
    out = perturb_unit(x, 2, seed=0, first=0)
    assert ((out.double().norm(dim=1) - 1).abs() <= 1e-6).all()


def test_perturb_unit_error_paths():
    from diffusion_pullback_amd import DpbError
    from diffusion_pullback_amd.engine import perturb_unit
    x = torch.zeros(16, device=DEV)
    with pytest.raises(DpbError, match="B=0"):
        perturb_unit(x, 0)
    with pytest.raises(DpbError, match="first"):
        perturb_unit(x, 1, first=-1)
    with pytest.raises(DpbError, match="noise has"):
        perturb_unit(x, 2, noise=torch.zeros(3, 16))
    assert perturb_unit(x, 2, seed=1).shape == (2, 16)


# ------------------------------------------------------------------ the reference's goldens, fp32 engine
def _check_against_case(c, u, s, bar_s=1e-4, bar_cos=0.9999):
    assert tuple(u.shape) == tuple(c["u"].shape) and tuple(s.shape) == (c["q"],)
    srel = ((s.double().cpu() - c["s"].double()).abs() / c["s"].double()).max().item()
    cos = abs_cos(u.T, c["u"].T)
    print("case", c["n"], c["memory_bound"], c["q"], "s rel", srel, "min |cos| u", cos.min().item())
    assert srel <= bar_s, (c["n"], c["q"], srel)
    assert cos.min() >= bar_cos, (c["n"], c["q"], cos)
    return torch.sign((u.T.double().cpu() * c["u"].T.double()).sum(-1))      # sign of every column against the reference's


@pytest.mark.parametrize("case", [0, 1, 2, 3])
def test_local_pca_zt_golden(case):
    """u and s of every case at the bars of test_global_pca_zt_golden (10x the conditioning the generator enforced).  vT: the product returns
    the x-direction of COLUMN i of u in row i -- what the issue specifies and what PullBackDDPM.inv_jac_xt computes -- while utils.local_pca_zt
    pairs its row i with row i of the row-major VIEW of u as [q, D] (utils.py:960; tests/_local_pca_ref.reference_pairing, shown on the fixture
    itself in test_local_pca_host.py).  At q = 1 the two coincide and the returned vT meets the fixture's directly.  At q > 1 the fixture's rows are
    met through the reference's own pairing: the method's u (signs aligned to the fixture's, which the mixture depends on) is re-paired and sent
    through the same adjoint path (inv_jac_zt, 2-D u); the returned vT is pinned to that path column by column.  Same bars, every row."""
    g, unet, _ = _sd()
    c = g["cases"][case]
    noise = position_at_R(c, tuple(g["z"].shape[1:]))          # seeds the global generator and consumes the reference's noise draws: R comes next
    u, s, vT = unet.local_pca_zt(g["z"], g["t"], g["ctx"], op=c["op"], block_idx=c["idx"], memory_bound=c["memory_bound"], num_pca_samples=c["n"],
                                 pca_rank=c["q"], noise=noise, perturb_h=c["perturb_h"])
    assert u.device.type == "cpu" and s.device.type == "cpu" and vT.device.type == "cpu" and u.dtype == torch.float32      # sample.device / dtype
    assert tuple(vT.shape) == tuple(c["vT"].shape)
    sign = _check_against_case(c, u, s)
    own = unet.inv_jac_zt(g["z"], g["t"], g["ctx"], op=c["op"], block_idx=c["idx"], u=u).cpu()
    assert abs_cos(vT, own).min() >= 0.999999 and ((vT * own).sum(-1) > 0).all()
    assert torch.allclose(vT.norm(dim=1), torch.ones(c["q"]), atol=1e-5)
    if c["q"] == 1:
        cos = abs_cos(vT, c["vT"])
        assert cos.min() >= 0.9999 and (sign * (vT.double() * c["vT"].double()).sum(-1) > 0).all(), cos
    W = reference_pairing((u.double() * sign).float())
    ref_rows = unet.inv_jac_zt(g["z"], g["t"], g["ctx"], op=c["op"], block_idx=c["idx"], u=W.T.contiguous()).cpu()
    cos = abs_cos(ref_rows, c["vT"])
    print("   min |cos| vT (reference pairing)", cos.min().item())
    assert cos.min() >= 0.9999 and ((ref_rows * c["vT"]).sum(-1) > 0).all(), cos


def test_local_pca_xt_golden():
    g, unet, _ = _ddpm()
    c = g["local"][0]
    noise = position_at_R(c, tuple(g["x"].shape[1:]))
    u, s, vT = unet.local_pca_xt(g["x"], g["t"], op=c["op"], block_idx=c["idx"], memory_bound=c["memory_bound"], num_pca_samples=c["n"],
                                 pca_rank=c["q"], noise=noise, perturb_h=c["perturb_h"])
    sign = _check_against_case(c, u, s)
    assert tuple(vT.shape) == tuple(c["vT"].shape)
    cos = abs_cos(vT, c["vT"])
    print("   min |cos| vT", cos.min().item())
    assert cos.min() >= 0.9999, cos
    assert (sign * (vT.double().cpu() * c["vT"].double()).sum(-1) > 0).all()       # the sign of vT is fixed relative to u


def test_global_pca_xt_and_inv_jac_xt_golden():
    g, unet, _ = _ddpm()
    c = g["global"][0]
    torch.manual_seed(c["rng_seed"])
    u, s = unet.global_pca_xt(c["x"], g["t"], op=c["op"], block_idx=c["idx"], memory_bound=c["memory_bound"], pca_rank=c["q"])
    assert u.device.type == "cpu"
    _check_against_case(c, u, s)
    for c in g["inv"]:
        vT = unet.inv_jac_xt(g["x"], g["t"], op=c["op"], block_idx=c["idx"], u=c["u"], perturb_h=c["perturb_h"])
        assert tuple(vT.shape) == tuple(c["vT"].shape)
        assert abs_cos(vT, c["vT"]).min() >= 0.9999 and ((vT.cpu() * c["vT"]).sum(-1) > 0).all(), c["name"]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_local_pca_runs_in_16_bit_engines(dtype):
    g, unet, _ = _sd(dtype)
    c = g["cases"][1]
    u, s, vT = unet.local_pca_zt(g["z"].to(DEV), g["t"], g["ctx"], op="mid", block_idx=0, memory_bound=c["memory_bound"], num_pca_samples=c["n"],
                                 pca_rank=c["q"], seed=5)
    assert tuple(u.shape) == (c["d"], c["q"]) and tuple(s.shape) == (c["q"],) and tuple(vT.shape) == (c["q"], 256)
    assert u.device.type == "cuda" and s.device.type == "cuda" and vT.device.type == "cuda" and u.dtype == torch.float32
    assert torch.isfinite(u).all() and torch.isfinite(s).all() and torch.isfinite(vT).all()
    assert (s[:-1] >= s[1:]).all() and (s > 0).all()


# ------------------------------------------------------------------ dpb_local_pca_sample in generated mode
def test_local_pca_sample_rows_are_forwards_of_the_perturbed_batch():
    from diffusion_pullback_amd.engine import perturb_unit
    g, _, impl = _sd(max_batch=5)
    eng, key, n = impl.engine, ("mid", 0), 12                      # chunks of 5, 5 and 2
    z, t, ctx = g["z"], float(g["t"]), g["ctx"]
    H = eng.local_pca_sample(z, t, ctx, key, n, seed=SEED, first=3)
    assert tuple(H.shape) == (n, 1024)
    for c0 in range(0, n, 5):
        b = min(5, n - c0)
        xb = perturb_unit(z.to(DEV), b, seed=SEED, first=3 + c0).view(b, *z.shape[1:])
        assert torch.equal(H[c0:c0 + b], eng.forward(xb, t, ctx, key).reshape(b, -1)), c0
    assert torch.equal(H, eng.local_pca_sample(z, t, ctx, key, n, seed=SEED, first=3))
    big = torch.zeros(n + 2, 1024, device=DEV)                     # rows of a caller's matrix, nothing written around them
    eng.local_pca_sample(z, t, ctx, key, n, seed=SEED, first=3, out=big[1:n + 1])
    assert torch.equal(big[1:n + 1], H) and not big[0].any() and not big[n + 1].any()
    # the engine's chunking does not change which noise a sample gets, nor -- beyond the rounding of a forward pass at another batch size -- its
    # features: fp32 products accumulate in fp32 (2^-24 per operation over sums of a few thousand terms), 1e-5 of the row's largest feature
    _, _, impl1 = _sd(max_batch=1)
    H1 = impl1.engine.local_pca_sample(z, t, ctx, key, n, seed=SEED, first=3)
    diff = ((H1 - H).abs().amax(dim=1) / H.abs().amax(dim=1)).max().item()
    print("max_batch 1 vs 5: bitwise", torch.equal(H1, H), "relative", diff)
    assert diff <= 1e-5, diff


# ------------------------------------------------------------------ method level, error paths, isolation
def test_local_pca_zt_seeded_calls_are_bitwise_equal_and_memory_bound_changes_nothing():
    g, unet, _ = _sd()
    kw = dict(op="mid", block_idx=0, num_pca_samples=20, pca_rank=4)
    res = []
    for mb, seed in ((5, 7), (5, 7), (4, 7)):
        torch.manual_seed(3)                                     # R
        res.append(unet.local_pca_zt(g["z"], g["t"], g["ctx"], memory_bound=mb, seed=seed, **kw))
    for r in res[1:]:
        for a, b in zip(res[0], r):
            assert torch.equal(a, b)
    torch.manual_seed(3)
    other = unet.local_pca_zt(g["z"], g["t"], g["ctx"], memory_bound=5, seed=8, **kw)
    assert not torch.equal(other[1], res[0][1])
    # seed=None: one draw from the global CPU generator, so torch.manual_seed governs the whole call
    torch.manual_seed(9)
    a = unet.local_pca_zt(g["z"], g["t"], g["ctx"], memory_bound=5, **kw)
    torch.manual_seed(9)
    b = unet.local_pca_zt(g["z"], g["t"], g["ctx"], memory_bound=5, **kw)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    u, s, vT = unet.local_pca_zt(g["z"], g["t"], g["ctx"], memory_bound=5, seed=7, return_x_direction=False, **kw)
    assert vT is None and tuple(u.shape) == (1024, 4)


def test_local_pca_error_paths_leave_the_engine_usable():
    from diffusion_pullback_amd import DpbError
    g, unet, impl = _sd()
    z, t, ctx = g["z"], g["t"], g["ctx"]
    with pytest.raises(ValueError, match="pca_rank"):
        unet.local_pca_zt(z, t, ctx, op="mid", block_idx=0, memory_bound=5, num_pca_samples=200, pca_rank=129)
    with pytest.raises(ValueError, match="multiple of memory_bound"):
        unet.local_pca_zt(z, t, ctx, op="mid", block_idx=0, memory_bound=7, num_pca_samples=40, pca_rank=4)
    with pytest.raises(ValueError, match="single sample"):
        unet.local_pca_zt(z.repeat(2, 1, 1, 1), t, ctx, op="mid", block_idx=0, memory_bound=5, num_pca_samples=40, pca_rank=4)
    with pytest.raises(ValueError, match="noise has shape"):
        unet.local_pca_zt(z, t, ctx, op="mid", block_idx=0, memory_bound=5, num_pca_samples=40, pca_rank=4, noise=torch.zeros(39, 4, 8, 8))
    with pytest.raises(ValueError, match="is not valid"):
        unet.local_pca_zt(z, t, ctx, op="mid", block_idx=3, memory_bound=5, num_pca_samples=40, pca_rank=4)
    # jvp after a local-PCA call is refused until the next primal
    impl.engine.primal(z, float(t), ctx, ("mid", 0))
    impl.engine.local_pca_sample(z, float(t), ctx, ("mid", 0), 3, seed=1)
    with pytest.raises(DpbError, match="dpb_primal must run"):
        impl.engine.jvp(("mid", 0), torch.zeros(1, 256))
    c = g["cases"][1]
    noise = position_at_R(c, tuple(z.shape[1:]))
    u, s, _ = unet.local_pca_zt(z, t, ctx, op="mid", block_idx=0, memory_bound=c["memory_bound"], num_pca_samples=c["n"], pca_rank=c["q"], noise=noise)
    assert abs_cos(u.T, c["u"].T).min() >= 0.9999


def test_pullback_bits_unchanged_by_a_local_pca_call():
    g, unet, impl = _sd()
    V0 = torch.linalg.qr(torch.randn(256, 3, generator=torch.Generator().manual_seed(41)))[0].T.contiguous()
    r1 = [t.clone() for t in impl.pullback_fixed(g["z"], g["t"], g["ctx"], "mid", 0, 3, 4, V0)]
    unet.local_pca_zt(g["z"], g["t"], g["ctx"], op="mid", block_idx=0, memory_bound=5, num_pca_samples=40, pca_rank=8, seed=2)
    r2 = impl.pullback_fixed(g["z"], g["t"], g["ctx"], "mid", 0, 3, 4, V0)
    for a, b in zip(r1, r2):
        assert torch.equal(a, b)


def test_bind_attaches_the_local_pca_family():
    _, unet, _ = _sd()
    assert callable(unet.local_pca_zt) and not hasattr(unet, "local_pca_xt")
    _, unet, _ = _ddpm()
    for name in ("local_pca_xt", "global_pca_xt", "inv_jac_xt"):
        assert callable(getattr(unet, name)), name
