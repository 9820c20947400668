"""The guided-diffusion (ADM) network kind on the GPU: PullbackUNet("adm", ...) against the REFERENCE's own UNetModel outputs (fixture
adm_toy.pt, tests/golden/make_golden_adm.py) and against the CPU restatement tests/_adm_ref.py (itself pinned to the reference by
tests/test_adm_host.py).  Toy configs T1 / T2 / T3 (tests/_adm_ref.py).  Bars are the project's own: relative Frobenius fp32 <= 2e-4, bf16 and
fp16 <= 4e-2."""
import pytest
import torch

import _adm_ref as R
from _util import abs_cos, load_golden, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF, F16 = torch.float32, torch.bfloat16, torch.float16
BAR = {F32: 2e-4, BF: 4e-2, F16: 4e-2}
_CACHE = {}


@pytest.fixture(scope="module")
def fix():
    return load_golden("adm_toy.pt")


def _params(name):
    from diffusion_pullback_amd import configs as cf
    if name not in _CACHE:
        _CACHE[name] = cf.adm_init_params(R.TOYS[name], **R.init_kwargs(R.TOY_INIT[name]))
    return _CACHE[name]


def _net(name, dtype, max_batch=2, max_rank=8, **kw):
    from diffusion_pullback_amd import PullbackUNet
    return PullbackUNet("adm", R.TOYS[name], _params(name), dtype=dtype, device=DEV, max_batch=max_batch, max_rank=max_rank, verbose=False, **kw)


# ----------------------------------------------------------------------------------------------- 1. primal
@pytest.mark.parametrize("name,dtype", [("T1", F32), ("T3", F32), ("T2", F32), ("T2", BF), ("T2", F16)],
                         ids=["T1-fp32", "T3-fp32", "T2-fp32", "T2-bf16", "T2-fp16"])
def test_primal_matches_the_reference(fix, name, dtype):
    """get_h (the middle block's output) and the full forward at batch 1 and 2 against the reference's own outputs"""
    f = fix["toys"][name]
    net = _net(name, dtype)
    for x, h, e in ((f["x"], f["h"], f["eps"]), (f["xb"], f["h_b"], f["eps_b"])):
        hh = net.get_h(x=x.to(DEV), t=f["t"])                       # UNetModel.get_h takes no (op, block_idx)
        ee = net(x.to(DEV), f["t"])
        assert hh.shape == h.shape and ee.shape == e.shape
        eh, eo = rel(hh, h), rel(ee, e)
        print(name, dtype, "batch", x.shape[0], "get_h", eh, "eps", eo)
        assert eh <= BAR[dtype] and eo <= BAR[dtype]
    assert torch.equal(net.get_h(x=f["x"].to(DEV), t=f["t"], op="mid", block_idx=0), net.get_h(x=f["x"].to(DEV), t=f["t"]))
    with pytest.raises(ValueError):
        net.get_h(x=f["x"].to(DEV), t=f["t"], op="down", block_idx=7)


# ----------------------------------------------------------------------------------------------- 2. tangent and adjoint
@pytest.mark.parametrize("name", ["T1", "T3"])
def test_tangent_and_adjoint_one_direction(fix, name):
    """x -> mid and the seeded mid -> eps pass (up ResBlocks, the nearest-up adjoint, the zeroed skip windows of the concats) against
    torch.func.jvp / vjp of the restatement, and <Ju, w> = <u, J^T w> to 1e-4 relative, fp32"""
    f, cfg, p = fix["toys"][name], R.TOYS[name], _params(name)
    net = _net(name, F32)
    eng = net.engine
    x, t = f["x"], f["t"]
    g = torch.Generator().manual_seed(11)
    eng.primal(x.to(DEV), 600.0, None, "eps")
    h = R.get_h(p, cfg, x, t).detach()
    for what, fn, x0, jvp, vjp in (
            ("x->mid", lambda a: R.get_h(p, cfg, a, t), x, lambda v: eng.jvp(("mid", 0), v), lambda w: eng.vjp(("mid", 0), w)),
            ("mid->eps", lambda a: R.get_h_to_e(p, cfg, x, t, a), h, lambda v: eng.jvp_between(("mid", 0), "eps", v),
             lambda w: eng.vjp_between(("mid", 0), "eps", w))):
        out, Ju_ref = torch.func.jvp(fn, (x0,), (u := torch.randn(x0.shape, generator=g),))
        w = torch.randn(out.shape, generator=g)
        (JTw_ref,) = torch.func.vjp(fn, x0)[1](w)
        Ju = jvp(u.reshape(1, -1).to(DEV)).cpu().reshape(out.shape)
        JTw = vjp(w.reshape(1, -1).to(DEV)).cpu().reshape(x0.shape)
        a, b = (Ju.double() * w.double()).sum().item(), (u.double() * JTw.double()).sum().item()
        print(name, what, "jvp", rel(Ju, Ju_ref), "vjp", rel(JTw, JTw_ref), "<Ju,w>", a, "<u,JTw>", b)
        assert rel(Ju, Ju_ref) <= BAR[F32] and rel(JTw, JTw_ref) <= BAR[F32]
        assert abs(a - b) <= 1e-4 * max(abs(a), abs(b))


# ----------------------------------------------------------------------------------------------- 3. indexing: per-sample timesteps
TS = [600.0, 123.0]


def _passes(net, x, t, V, U):
    """primal, tangent and adjoint at mid and eps of a batch of 2 with k = 3 directions per sample, and the launches of each pass"""
    eng = net.engine
    out, n = {}, {}
    for tap in (("mid", 0), "eps"):
        eng.primal(x, t, None, tap)
        n[(tap, "primal")] = eng.stats()[0]
        out[(tap, "primal")] = eng.read(tap).clone()
        out[(tap, "tangent")] = eng.jvp(tap, V).clone()
        n[(tap, "tangent")] = eng.stats()[0]
        out[(tap, "adjoint")] = eng.vjp(tap, U[tap]).clone()
        n[(tap, "adjoint")] = eng.stats()[0]
    return out, n


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_rows_of_a_mixed_timestep_batch_are_bitwise_the_scalar_runs(fix, dtype):
    """Batch 2, k = 3 tangents per sample, DISTINCT timesteps: each row of primal, tangent and adjoint is bitwise the row of the same batch at
    that row's scalar timestep (the invariant tests/test_gpu_timesteps.py pins for the other kinds), at mid and eps.  Equal timesteps passed
    per sample are the scalar call launch for launch and bit for bit."""
    f = fix["toys"]["T1"]
    net = _net("T1", dtype, max_batch=2, max_rank=6)
    x = f["xb"].to(DEV)
    g = torch.Generator().manual_seed(3)
    V = torch.randn(6, x[0].numel(), generator=g).to(DEV)
    U = {tap: torch.randn(6, net.engine.tap_numel(tap), generator=g).to(DEV) for tap in (("mid", 0), "eps")}
    het, _ = _passes(net, x, torch.tensor(TS), V, U)
    refs = [_passes(net, x, TS[i], V, U) for i in range(2)]
    for key, a in het.items():
        assert torch.isfinite(a).all(), key
        per = a.shape[0] // 2
        for i in range(2):
            r = refs[i][0][key]
            assert torch.equal(a[i * per:(i + 1) * per], r[i * per:(i + 1) * per]), \
                f"{key} sample {i}: max |d| = {(a[i * per:(i + 1) * per] - r[i * per:(i + 1) * per]).abs().max().item():.3e}"
    assert not torch.equal(refs[0][0][("eps", "primal")][1], refs[1][0][("eps", "primal")][1])     # the timestep matters
    assert not torch.equal(refs[0][0][(("mid", 0), "tangent")][3:], refs[1][0][(("mid", 0), "tangent")][3:])
    same, n_same = _passes(net, x, torch.tensor([TS[0], TS[0]]), V, U)
    for key, a in same.items():
        assert torch.equal(a, refs[0][0][key]), key
        assert n_same[key] == refs[0][1][key], (key, n_same[key], refs[0][1][key])


# ----------------------------------------------------------------------------------------------- 4. pullback
def test_pullback_matches_the_reference_function(fix):
    """local_encoder_pullback_xt on T1, k = 3, V0 drawn under the recorded seed, against (s, vT) RETURNED BY THE REFERENCE CLASS'S OWN
    local_encoder_pullback_xt (unet.py:704-781), at the per-vector bar of test_ddpm256_headline_vs_reference_function_golden (fp32: s to
    rtol 1e-3, |cos| > 0.9999).  |cos| is asked of the vectors whose singular value is separated from both neighbours by more than 5 % in the
    fp64 SVD of the restatement's full Jacobian; at least two of the three must be.  Then k = 8 against that SVD."""
    f, cfg = fix["toys"]["T1"], R.T1
    sv, Vh = R.full_jacobian_svd(f, cfg)
    ok = R.separated(sv, 3)
    assert sum(ok) >= 2, (sv[:5], ok)
    net = _net("T1", F32, max_batch=1, max_rank=8, upto=("mid", 0))
    x = f["x"].to(DEV)
    torch.manual_seed(fix["rng_seed"])
    u, s, vT = net.local_encoder_pullback_xt(x, f["t"], op="mid", block_idx=0, pca_rank=fix["k"], chunk_size=fix["chunk_size"],
                                             min_iter=fix["min_iter"], max_iter=fix["max_iter"], convergence_threshold=fix["thr"])
    assert net.last_iters == f["iters"]
    cos = abs_cos(vT.cpu(), f["vT"])
    print("s", s.tolist(), "reference", f["s"].tolist(), "|cos|", cos.tolist(), "separated", ok)
    assert torch.allclose(s.cpu(), f["s"], rtol=1e-3), (s, f["s"])
    assert all(c > 0.9999 for c, o in zip(cos.tolist(), ok) if o), (cos, ok)
    assert torch.allclose(u.cpu().norm(dim=0), f["u_norms"], rtol=1e-3)
    V0 = torch.linalg.qr(torch.randn(x[0].numel(), 8, generator=torch.Generator().manual_seed(8)))[0].T.contiguous()
    u, s, vT = net.local_encoder_pullback_xt(x, f["t"], op="mid", block_idx=0, pca_rank=8, chunk_size=5, min_iter=10, max_iter=60,
                                             convergence_threshold=1e-5, V0=V0)
    assert torch.allclose(s.cpu()[:4].double(), sv[:4], rtol=2e-3), (s[:4], sv[:4])
    assert torch.allclose((vT @ vT.T).cpu(), torch.eye(8), atol=1e-3)
    assert (abs_cos(vT[:3].cpu(), Vh[:3].float()) > 0.99).all()


# ----------------------------------------------------------------------------------------------- 5. shifted forward
def test_shifted_forward_with_a_shared_prefix(fix):
    """The h-space shift at ('mid', 0) with ONE x and three (direction, scale) rows (dpb_forward_shift's shared prefix, and h_traversal on top of
    it): the part of the net up to the tap runs once at batch 1, so the affine tables of the modulated GroupNorms after it must have been filled
    for all three rows -- against the restatement's get_h_to_e(h + s u).  Then unet(x, t, u=, op='mid', block_idx=0) itself, one u broadcast
    over a batch of 2."""
    f, cfg, p = fix["toys"]["T1"], R.T1, _params("T1")
    net = _net("T1", F32, max_batch=3, max_rank=3)
    x, t = f["x"], f["t"]
    h = R.get_h(p, cfg, x, t)
    d = h[0].numel()
    g = torch.Generator().manual_seed(21)
    U = torch.randn(d, 2, generator=g)
    rows = [(0, 1.5), (1, -2.0), (0, -0.5)]
    Ud = (U / U.norm(dim=0, keepdim=True)).T.contiguous().to(DEV)
    out = net.engine.forward_shift(x.to(DEV), 600.0, None, ("mid", 0), Ud, [r[0] for r in rows], [r[1] for r in rows], "eps")
    grid = net.h_traversal(x.to(DEV), t, None, U.to(DEV), [1.5, -2.0], "mid", 0)          # 2 directions x 2 scales: chunks of 3 + 1 rows
    assert rel(grid[0, 0], out[0]) <= 1e-5 and rel(grid[1, 1], out[1]) <= 1e-5          # (other batch compositions: other tiles, fp32 noise)
    Un = U / U.norm(dim=0, keepdim=True)
    with torch.no_grad():
        for b, (i, sc) in enumerate(rows):
            ref = R.get_h_to_e(p, cfg, x, t, h + sc * Un[:, i].reshape(h.shape))
            e = rel(out[b:b + 1], ref)
            print("shift row", b, e)
            assert e <= BAR[F32]
        u1 = 0.5 * h.std() * torch.randn(h.shape, generator=g)
        eb = net(f["xb"].to(DEV), t, u=u1.to(DEV), op="mid", block_idx=0)
        hb = R.get_h(p, cfg, f["xb"], t)
        for b in range(2):
            ref = R.get_h_to_e(p, cfg, f["xb"][b:b + 1], t, hb[b:b + 1] + u1)
            assert rel(eb[b:b + 1], ref) <= BAR[F32]


def test_bind_attaches_the_uncond_surface(fix):
    """bind(unet, 'adm'): the state dict's names are the parameter names; the DDPM-kind methods are attached"""
    from diffusion_pullback_amd import bind
    f = fix["toys"]["T3"]

    class Holder:                                        # stands for the reference module: only state_dict() is read
        def state_dict(self):
            return _params("T3")
    m = Holder()
    impl = bind(m, "adm", R.T3, dtype=F32, device=DEV, max_batch=1, max_rank=3, verbose=False)
    assert impl.kind == "adm"
    for name in ("get_h", "get_h_to_e", "local_encoder_pullback_xt", "local_decoder_pullback_xt", "local_pca_xt", "global_pca_xt", "inv_jac_xt"):
        assert hasattr(m, name), name
    assert rel(m.get_h(x=f["x"].to(DEV), t=f["t"]), f["h"]) <= BAR[F32]
