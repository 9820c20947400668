"""The pullback geodesic without a GPU: the references of tests/_geodesic_ref.py against what a geodesic must be (a linear map: the uniform straight
line; a rank-deficient one: the unseen components stay), the formula g_i = J^T c_i + lam d_i of the kernel restatements against autograd of the energy
on the oracle's toy nets in float64, the block driver's rules, the argument checks of pullback_geodesic / curve_energy / the command line, and the
exported symbols against the header.  (The kernels: tests/test_gpu_geodesic_ops.py; the chain: tests/test_gpu_geodesic_chain.py.)"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import _geodesic_ref as R

F64 = torch.float64


def _linear(A):
    return lambda x: x.flatten(1) @ A.T


def _map(D, N, sv, seed):
    """A [D, N] with the singular values sv (zeros allowed): A = Q_D diag(sv) Q_N^T"""
    g = torch.Generator().manual_seed(seed)
    q1, _ = torch.linalg.qr(torch.randn(D, D, generator=g, dtype=F64))
    q2, _ = torch.linalg.qr(torch.randn(N, N, generator=g, dtype=F64))
    S = torch.zeros(D, N, dtype=F64)
    S[range(len(sv)), range(len(sv))] = torch.tensor(sv, dtype=F64)
    return q1 @ S @ q2.T


def _ends(seed, shape=(1, 2, 3)):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=F64), torch.randn(*shape, generator=g, dtype=F64)


def _start(xa, xb, m, init):
    from diffusion_pullback_amd.pullback import geodesic_init
    P = geodesic_init(xa.float(), xb.float(), m, init).double()
    P[0], P[-1] = xa, xb                                            # (the float64 ends, not their fp32 roundings)
    return P


def test_linear_map_converges_to_the_uniform_straight_line():
    """(a) h = A x with A injective: E is a convex quadratic whose minimiser is the uniform straight line, whatever the start"""
    m, N = 3, 6
    A = _map(9, N, [1.0, 1.2, 1.4, 1.6, 1.8, 2.0], 0)
    xa, xb = _ends(1)
    P0 = _start(xa, xb, m, "slerp")
    curve, info = R.descent_ref(_linear(A), P0, 0.0, None, max_iter=4000, tol=0.0, check_every=50)
    s = (torch.arange(m + 2, dtype=F64) / (m + 1)).view(-1, 1, 1, 1)
    line = xa + s * (xb - xa)
    assert float((curve - line).abs().max()) <= 1e-8, float((curve - line).abs().max())
    want = float((A @ (xb - xa).reshape(-1)).pow(2).sum()) / (2 * (m + 1))
    assert abs(info["energy"][-1] - want) <= 1e-10 * want and abs(info["energy_h"] - want) <= 1e-10 * want
    assert info["energy"][-1] < info["start"]["energy"] and abs(info["uniformity"] - 1) <= 1e-12
    assert torch.equal(curve[0], xa) and torch.equal(curve[-1], xb)
    assert info["monotone"]
    # (at the minimum E moves by its own rounding only: no rise INSIDE a block is claimed for the descent before that, 100 iterations of it)
    assert R.descent_ref(_linear(A), P0, 0.0, None, max_iter=100, tol=0.0, check_every=50)[1]["rises"] == 0


def test_rank_deficient_map_keeps_what_it_does_not_see():
    """(a) lam = 0 with N_h < N_in: g_i lies in the row space of A, so the null-space components of the slerp start are unchanged"""
    m, N = 3, 6
    A = _map(4, N, [1.0, 1.5, 2.0, 0.0], 2)                          # rank 3
    xa, xb = _ends(3)
    P0 = _start(xa, xb, m, "slerp")
    curve, info = R.descent_ref(_linear(A), P0, 0.0, None, max_iter=400, tol=0.0, check_every=20)
    null = torch.eye(N, dtype=F64) - torch.linalg.pinv(A) @ A
    moved = (curve - P0).flatten(1)
    assert float((moved @ null.T).abs().max()) <= 1e-12
    assert float(moved.abs().max()) > 1e-3 and info["energy"][-1] < info["start"]["energy"]


def _toy(kind, m):
    """(get_hs float64, P [m + 2, ...] float64, t) on the oracle toy nets"""
    import test_gpu_inv_jac_chain as IJ
    _, _, x, ctx = IJ._model(kind)
    P = _start(x[0].double(), x[1].double(), m, "slerp")
    P[1:-1] += 0.05 * torch.randn(P[1:-1].shape, generator=torch.Generator().manual_seed(7), dtype=F64)
    c = None if ctx is None else torch.cat([ctx, ctx[:m - 1] + 0.1])[:m + 2]
    return R.get_hs(kind, ("mid", 0), F64, 301.0, c), P, c


@pytest.mark.parametrize("kind", ["ddpm", "adm", "sd"])
def test_formula_of_the_restatements_is_the_gradient_of_the_energy(kind):
    """(b) g_i = J(P_i)^T (2 h_i - h_{i-1} - h_{i+1}) + lam (2 P_i - P_{i-1} - P_{i+1}), through the float64 forms of the two kernel restatements and
    the oracle's vjp_step, against autograd of E itself: relative 1e-12"""
    from oracle.pullback import vjp_step
    m, lam = 2, 0.3
    g, P, _ = _toy(kind, m)
    gh, gx, seg_h, seg_x = R.gradients(g, P)
    with torch.no_grad():
        h = R._h_of(g, P)
    cot, seg, csq = R.cotangents_ref(h.numpy(), round32=False)
    assert np.allclose(seg, seg_h.numpy(), rtol=1e-13, atol=0)
    one = lambda i: g[i] if isinstance(g, list) else g
    hs = one(1)(P[1:2]).shape
    W = torch.cat([vjp_step(one(i + 1), P[i + 1:i + 2], torch.from_numpy(cot[i]).reshape(1, *hs[1:])) for i in range(m)])
    out, stats, xseg = R.update_ref(P.flatten(1).numpy(), W.numpy(), 1.0, lam, round32=False)
    got = torch.from_numpy(P.flatten(1).numpy()[1:-1] - out[1:-1])               # eta = 1: the step IS g
    want = gh + lam * gx
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= 1e-12 * scale, (float((got - want).abs().max()), scale)
    assert np.allclose(stats[:, 0], (gh * gh).sum(1).numpy(), rtol=1e-11) and np.allclose(stats[:, 1], (want * want).sum(1).numpy(), rtol=1e-11)
    assert np.allclose(xseg, seg_x.numpy(), rtol=1e-13) and (stats[:, 3] == 0).all()
    r = R.geodesic_ref(g, P, 1e-3, lam, 1)                                       # and the chain reference's own records
    assert np.allclose(r["csq"][0].numpy(), csq, rtol=1e-12) and np.allclose(r["stats"][0, :, 1].numpy(), stats[:, 1], rtol=1e-11)


def test_restatements_edge_cases():
    rng = np.random.default_rng(0)
    P, W = rng.integers(-8, 8, (4, 5)).astype(np.float32), rng.integers(-8, 8, (2, 5)).astype(np.float32)
    out, stats, xseg = R.update_ref(P, W, 0.0, 0.5)
    assert out.tobytes() == P.tobytes() and (stats[:, 2] == 0).all()
    out, stats, xseg = R.update_ref(P, W, 0.25, 0.5)
    d = 2 * P[1:-1] - P[:-2] - P[2:]
    assert np.array_equal(out[1:-1], P[1:-1] - 0.25 * (W + 0.5 * d)) and np.array_equal(out[[0, -1]], P[[0, -1]])
    assert np.array_equal(xseg, ((P[1:] - P[:-1]) ** 2).sum(1))
    W[1, 2] = np.nan
    out, stats, _ = R.update_ref(P, W, 0.25, 0.5)
    assert stats[:, 3].tolist() == [0.0, 1.0] and np.isnan(out[2]).all() and np.isfinite(out[[0, 1, 3]]).all()
    cot, seg, csq = R.cotangents_ref(P)
    assert np.array_equal(cot, d) and np.array_equal(csq, (d.astype(np.float64) ** 2).sum(1)) and cot.dtype == np.float32


def test_driver_rejects_too_large_a_step_and_gives_up_after_max_halvings():
    """(c) eta 100x the step rule: the first block is rejected and eta halved until a block descends; with max_halvings too few: converged False"""
    m = 3
    A = _map(9, 6, [1.0, 1.2, 1.4, 1.6, 1.8, 2.0], 0)
    xa, xb = _ends(1)
    P0 = _start(xa, xb, m, "slerp")
    g = _linear(A)
    eta0 = R.step_rule(R.geodesic_ref(g, P0, 0.0, 0.0, 1, F64, False))
    curve, info = R.descent_ref(g, P0, 0.0, 100 * eta0, max_iter=200, tol=1e-6, check_every=4, max_halvings=12)
    k = info["decisions"].index(True)
    assert k >= 3 and not any(info["decisions"][:k]) and info["halvings"] >= k and info["monotone"]
    assert info["step_size"] == 100 * eta0 / 2 ** info["halvings"] and info["energy"][-1] < info["start"]["energy"]
    assert info["attempted"] == 4 * len(info["decisions"]) or info["attempted"] == 200
    assert info["iterations"] == 4 * sum(info["decisions"]) or info["attempted"] == 200
    curve2, info2 = R.descent_ref(g, P0, 0.0, 100 * eta0, max_iter=200, tol=1e-6, check_every=4, max_halvings=2)
    assert info2["converged"] is False and info2["halvings"] == 2 and info2["decisions"] == [False, False] and info2["iterations"] == 0
    assert torch.equal(curve2, P0) and info2["energy"] == [info2["start"]["energy"]]
    # the product's driver on the same blocks takes the same decisions
    from diffusion_pullback_amd.pullback import geodesic_descent

    def block(P, eta, iters, final):
        r = R.geodesic_ref(g, P, eta, 0.0, iters, F64, final)
        return r["curves"], r["seg_h"], r["seg_x"], r["stats"], r["csq"]
    for kw in (dict(max_halvings=12), dict(max_halvings=2)):
        ref_curve, ref = R.descent_ref(g, P0, 0.0, 100 * eta0, max_iter=200, tol=1e-6, check_every=4, **kw)
        got_curve, got = geodesic_descent(block, P0, 0.0, 100 * eta0, 200, 1e-6, 4, kw["max_halvings"])
        assert torch.equal(got_curve, ref_curve)
        for key in ("decisions", "halvings", "iterations", "attempted", "converged", "monotone", "rises", "energy", "step_size", "length_h", "uniformity"):
            assert got[key] == ref[key], key
    got_curve, got = geodesic_descent(block, P0, 0.0, None, 40, 1e-6, 4, 8)        # the probe: the step rule
    ref_curve, ref = R.descent_ref(g, P0, 0.0, None, max_iter=40, tol=1e-6, check_every=4)
    assert torch.equal(got_curve, ref_curve) and got["step_size"] == ref["step_size"] and got["decisions"] == ref["decisions"]


class _StubEngine:
    """what the argument checks read of an engine; any pass would raise AttributeError"""
    def __init__(self, max_batch=5, max_tangents=3):
        self.max_batch, self.max_tangents = max_batch, max_tangents
        self.tape = type("T", (), {"taps": {("mid", 0): 0}})()

    def tap_numel(self, key):
        return 12


def _stub(kind="ddpm", **kw):
    from diffusion_pullback_amd import PullbackUNet
    n = PullbackUNet.__new__(PullbackUNet)
    n.kind, n.engine, n.in_shape, n.device = kind, _StubEngine(**kw), (3, 4, 4), torch.device("cpu")
    return n


def test_argument_validation_needs_no_gpu():
    """(d) every refusal of pullback_geodesic and curve_energy comes before anything runs (the stub has no passes)"""
    net = _stub()
    xa, xb = torch.randn(1, 3, 4, 4), torch.randn(1, 3, 4, 4)
    geo = lambda **k: net.pullback_geodesic(**{**dict(x_a=xa, x_b=xb, t=301.0, n_points=3, op="mid", block_idx=0), **k})
    for kw, word in ((dict(n_points=0), "n_points=0"), (dict(n_points=4), "max_batch=5"), (dict(lam=-0.1), "lam="), (dict(lam=float("nan")), "lam="),
                     (dict(init="cubic"), "init"), (dict(init=torch.zeros(4, 3, 4, 4)), "init has shape"), (dict(init=torch.zeros(5, 3, 4, 4)), "end rows"),
                     (dict(x_a=torch.randn(2, 3, 4, 4)), "one sample"), (dict(x_b=torch.randn(1, 3, 5, 4)), "one sample"), (dict(x_a=None), "x_a and x_b"),
                     (dict(step_size=0.0), "step_size"), (dict(step_size=float("inf")), "step_size"), (dict(max_iter=0), "max_iter"),
                     (dict(check_every=0), "check_every"), (dict(tol=-1.0), "tol="), (dict(max_halvings=-1), "max_halvings"),
                     (dict(encoder_hidden_states=torch.zeros(2, 5, 16)), "encoder_hidden_states has 2 rows"),
                     (dict(t=[301.0, 302.0, 301.0, 301.0, 301.0]), "one timestep"), (dict(op="nowhere"), "not valid")):
        with pytest.raises(ValueError, match=re.escape(word)):
            geo(**kw)
    with pytest.raises(ValueError, match="max_rank=3"):
        _stub(max_batch=8).pullback_geodesic(x_a=xa, x_b=xb, t=301.0, n_points=4, op="mid", block_idx=0)
    with pytest.raises(AttributeError):                                            # valid arguments reach the engine (which the stub lacks)
        geo()
    with pytest.raises(AttributeError):
        geo(x_a=xa[0], x_b=xb[0], init="linear", encoder_hidden_states=torch.zeros(1, 5, 16))
    en = lambda **k: net.curve_energy(**{**dict(curve=torch.randn(5, 3, 4, 4), t=301.0, op="mid", block_idx=0), **k})
    for kw, word in ((dict(curve=torch.randn(6, 3, 4, 4)), "max_batch=5"), (dict(curve=torch.randn(2, 3, 4, 4)), "n_points=0"),
                     (dict(curve=torch.randn(5, 3, 4)), "curve must be"), (dict(curve=None), "curve must be"), (dict(lam=-1.0), "lam="),
                     (dict(encoder_hidden_states=torch.zeros(3, 5, 16)), "encoder_hidden_states has 3 rows")):
        with pytest.raises(ValueError, match=re.escape(word)):
            en(**kw)


def test_start_curves():
    from diffusion_pullback_amd.pullback import geodesic_init
    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(3, 4, 4, generator=g), torch.randn(3, 4, 4, generator=g)
    for init in ("slerp", "linear"):
        P = geodesic_init(a, b, 4, init)
        assert P.shape == (6, 3, 4, 4) and P.dtype == torch.float32 and torch.equal(P[0], a) and torch.equal(P[-1], b)
    lin = geodesic_init(a, b, 4, "linear")
    assert torch.allclose(lin[2], a + 0.4 * (b - a), atol=1e-6)
    sl = geodesic_init(a, b, 4, "slerp")
    w = math.acos(float((a * b).sum() / (a.norm() * b.norm())))
    assert torch.allclose(sl[2], (math.sin(0.6 * w) * a + math.sin(0.4 * w) * b) / math.sin(w), atol=1e-6)
    assert torch.equal(geodesic_init(a, a, 2, "slerp"), a.expand(4, -1, -1, -1))  # no angle: the linear form
    assert geodesic_init(a, b, 4, sl) is not None and torch.equal(geodesic_init(a, b, 4, sl), sl)


def _parse(*argv):
    from diffusion_pullback_amd.main import parse_args
    return parse_args(["--note", "n", *argv])


def test_cli_flags_and_parser_errors():
    from diffusion_pullback_amd.main import _FLAGS
    from diffusion_pullback_amd.edit import EditStableDiffusion, EditUncondDiffusion
    a = _parse()
    assert (a.run_geodesic_interpolation, a.geodesic_points, a.geodesic_lambda, a.geodesic_max_iter, a.geodesic_tol) == (False, 8, 0.0, 200, 1e-4)
    assert {"run_geodesic_interpolation", "geodesic_points", "geodesic_lambda", "geodesic_max_iter", "geodesic_tol"} <= {f[0] for f in _FLAGS}
    job = ("--run_geodesic_interpolation", "True", "--sample_idx_0", "0", "--sample_idx_1", "1")
    for model in ("CelebA_HQ_HF", "runwayml/stable-diffusion-v1-5"):                # both drivers: the job has no reason to refuse SD
        ok = _parse(*job, "--model_name", model, "--geodesic_points", "5", "--geodesic_lambda", "0.5", "--geodesic_max_iter", "12", "--geodesic_tol", "1e-3")
        assert (ok.geodesic_points, ok.geodesic_lambda, ok.geodesic_max_iter, ok.geodesic_tol) == (5, 0.5, 12, 1e-3)
    for argv in ((*job, "--geodesic_points", "0"), (*job, "--geodesic_lambda", "-1"), (*job, "--geodesic_lambda", "nan"),
                 ("--run_geodesic_interpolation", "True", "--sample_idx_0", "2", "--sample_idx_1", "2"), ("--run_geodesic_interpolation", "True"),
                 (*job, "--geodesic_max_iter", "0"), (*job, "--geodesic_tol", "-1")):
        with pytest.raises(SystemExit):
            _parse(*argv)
    assert _parse("--geodesic_points", "0").geodesic_points == 0                   # the flags are checked for the job only
    for cls in (EditStableDiffusion, EditUncondDiffusion):
        assert callable(cls.run_geodesic_interpolation) and callable(cls._geodesic_decode) and callable(cls._geodesic_ctx)


NAMES = ("dpb_geodesic_cotangents_scratch_bytes", "dpb_geodesic_cotangents", "dpb_geodesic_update_scratch_bytes", "dpb_geodesic_update",
         "dpb_geodesic_chain_scratch_bytes", "dpb_geodesic_chain")
CTYPES = {"int": C.c_int, "float": C.c_float, "int64_t": C.c_int64, "size_t": C.c_size_t}


def _header_signature(header, name):
    """(restype, argtypes) of a prototype of include/dpb.h in ctypes terms: every pointer is a void pointer"""
    m = re.search(r"^(\w+)\s+" + name + r"\(([^;]*)\);", header, re.M)
    assert m, name
    args = [re.sub(r"/\*.*?\*/", "", a, flags=re.S).strip() for a in m.group(2).split(",")]
    typ = lambda a: C.c_void_p if "*" in a else CTYPES[a.replace("const ", "").split()[0]]
    return CTYPES[m.group(1)], [typ(a) for a in args]


def test_new_symbols_are_declared_with_the_headers_signatures():
    """(e) lib.SYMBOLS against include/dpb.h, argument by argument, and the bound library"""
    import inspect
    from diffusion_pullback_amd import PullbackUNet, engine, lib, pullback
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dpb.h")).read()
    for n in NAMES:
        assert n in lib.SYMBOLS, n
        res, args = _header_signature(header, n)
        assert lib.SYMBOLS[n][0] is res and list(lib.SYMBOLS[n][1]) == args, n
    L = lib.load()                                                # binds every declared symbol: a missing one raises
    assert L.dpb_abi_version() == 1
    assert L.dpb_geodesic_cotangents_scratch_bytes(3, 4097) == 4 * 2 * 2 * 8 and L.dpb_geodesic_cotangents_scratch_bytes(0, 5) == 0
    assert L.dpb_geodesic_update_scratch_bytes(3, 4097) == 4 * 2 * 5 * 8 and L.dpb_geodesic_update_scratch_bytes(3, 0) == 0
    assert L.dpb_geodesic_update_scratch_bytes(32767, 4) == 0 and L.dpb_geodesic_chain_scratch_bytes(None, 1, 1) == 0
    assert callable(engine.geodesic_cotangents) and callable(engine.geodesic_update) and callable(engine.Engine.geodesic_chain)
    sig = inspect.signature(PullbackUNet.pullback_geodesic).parameters
    for a, d in (("x_a", None), ("x_b", None), ("t", None), ("n_points", 8), ("op", None), ("block_idx", None), ("encoder_hidden_states", None),
                 ("init", "slerp"), ("lam", 0.0), ("step_size", None), ("max_iter", 200), ("tol", 1e-4), ("check_every", 4), ("max_halvings", 8), ("check", True)):
        assert a in sig and sig[a].default == d, a
    assert callable(PullbackUNet.curve_energy) and "pullback_geodesic" in inspect.getsource(pullback.bind) and "curve_energy" in inspect.getsource(pullback.bind)


def test_host_side_refusals_need_no_gpu():
    """the two kernels' entry points validate their host arguments before anything is launched (device pointers: a dummy non-null value, never read)"""
    from diffusion_pullback_amd import lib
    L = lib.load()
    err = lambda: L.dpb_last_error()
    cot = lambda **k: L.dpb_geodesic_cotangents(k.get("h", 8), k.get("cot", 8), k.get("seg", 8), k.get("csq", None), k.get("m", 2), k.get("D", 4),
                                                k.get("scratch", 256), k.get("bytes", 1 << 20), None)
    upd = lambda **k: L.dpb_geodesic_update(k.get("P", 4096), k.get("W", 8), k.get("out", 1 << 20), k.get("eta", 0.1), k.get("lam", 0.0), k.get("m", 2),
                                            k.get("N", 4), k.get("stats", 8), k.get("xseg", 8), k.get("scratch", 256), k.get("bytes", 1 << 20), None)
    for call in (cot, upd):
        assert call(m=0) != 0 and b"m=0" in err()
        assert call(m=32767) != 0 and b"m=32767" in err()
        assert call(bytes=8) != 0 and b"scratch of" in err()
        assert call(scratch=260) != 0 and b"aligned" in err()
    assert cot(D=0) != 0 and b"row length 0" in err() and upd(N=0) != 0 and b"row length 0" in err()
    for kw in (dict(h=None), dict(cot=None), dict(seg=None), dict(scratch=None)):
        assert cot(**kw) != 0 and b"null" in err(), kw
    for kw in (dict(P=None), dict(W=None), dict(out=None), dict(stats=None), dict(xseg=None), dict(scratch=None)):
        assert upd(**kw) != 0 and b"null" in err(), kw
    for kw in (dict(eta=float("nan")), dict(eta=float("inf")), dict(lam=float("nan")), dict(lam=-0.5)):
        assert upd(**kw) != 0 and b"finite" in err(), kw
    assert upd(out=4096) != 0 and b"overlaps" in err()
    assert upd(out=4096 + 4 * 4 * 3) != 0 and b"overlaps" in err()               # P_out starting inside P
    assert L.dpb_geodesic_chain(None, 0, 8, 1, 1.0, None, 0.1, 0.0, 1, 1, 8, 8, 8, 8, None, 8, 1 << 20) != 0 and b"null" in err()
