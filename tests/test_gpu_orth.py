"""dpb_orth (csrc/orth.hip) on the GPU against numpy.linalg.svd in float64, route by route.

Measures and bounds are those of tests/_orth_ref.py, in units of the per-case FLOOR (the error of the float64 reference rounded to fp32): vec = worst
row ||V[i] - V_ref[i]|| / floor, on = max|V V^T - I| / floor, s_ulps = |s - sqrt(S)| in fp32 ulps, conv0_ulps / conv1_err against a float64
recomputation from the returned V.  Bounds: vec, on <= 2 up to three decades of singular values, <= 4 at four; s_ulps <= 1; conv0_ulps <= 1;
conv1_err <= 2^-23 max|V - Vprev|.  tests/test_orth_host.py holds the float64 restatement of the method to the same bounds and keeps two fp32 mutants
(Gram matrix, V = Cm W) failing vec by 16x and more.  Every case prints `ORTH-ERR k N decades route vec on s_ulps conv0_ulps conv1_err`.

Pinned domain: the method squares the condition number (Gram matrix), so full fp32 accuracy holds up to cond(W) ~ 1e4.  Five and six decades are run
and recorded, not pinned: there eps64 cond^2 exceeds the fp32 floor and the float64 restatement itself leaves the bounds (vec 18 and 1200).

Near rank deficiency the trailing singular values are rounding noise of the fp32 rows (~1e-8 of the leading ones; their Gram eigenvalues ~1e-16, at
the float64 resolution of the Gram matrix): the trailing s and rows are only required finite, s >= 0.

Measured maxima on an MI355X per route (vec | on | s_ulps | conv0_ulps | conv1_err); no bound needed raising:
    apply16     (k 1 .. 16)                  1.000 | 1.000 | 0.423 | 0.192 | 6.9e-09
    apply56     (k 17 .. 56)                 1.000 | 1.000 | 0.483 | 0.256 | 6.5e-09
    tiled       (k 57, 64)                   1.000 | 1.000 | 0.442 | 0.366 | 5.8e-09
    eig96       (k 65, 96)                   1.000 | 1.000 | 0.438 | 0.252 | 6.0e-09
    qglobal     (k 97, 128)                  1.000 | 1.000 | 0.474 | 0.049 | 6.7e-09
    gridstride  (N = 65795)                  1.000 | 1.001 | 0.457 | 0.224 | 6.8e-10
    ladder      (50 x 16384) 1 .. 3 decades  1.000 | 1.000 | 0.439 | 0.378 | 1.8e-09
    ladder      4 decades                    1.025 | 1.000 | 0.437 | 0.379 | 7.4e-10
    converged   (k 5, 50, 128)               1.000 | 1.000 | 0.467 | 0.293 | 1.9e-17
    dead        (k 5, 12, 40, 100)           1.000 | 1.000 | 0.457 | 0.313 | 8.5e-09
    deficient   (k 12, 50), leading k - 2    1.000 | 1.000 | 0.419 | 0.202 | 3.5e-09     trailing s 9e-05 .. 1.6e-04 against a leading 1.0
    batched     (B 3 | 2, N = 640)           1.000 | 1.000 | 0.477 | 0.430 | 9.4e-09     singular values of W over 1.1x .. 3.4x
    cyclic      (DPB_EIG_PAR=0; 6 .. 56)     1.000 | 1.000 | 0.446 | 0.292 | 7.1e-09
    roundrobin  (DPB_EIG_PAR=2; 1, 2, 5)     1.000 | 1.000 | 0.153 | 0.267 | 6.0e-09
  outside the pinned domain (recorded, not asserted beyond finiteness and the leading half of s):
    5 decades                                12.09 | 181.5 | 0.421 | 0.182 | 1.4e-09
    6 decades                                1126  | 9201  | 15.33 | 0.182 | 1.7e-09     (s_ulps of the leading half: < 1)
Bitwise: two calls, the in-place call and the batched launch of dpb_pullback_iterate all return the bits of the single out-of-place call.

Non-finite input (the rule of include/dpb.h, exact: NaN masks and bit equality, no tolerance):
  * a NaN or an inf anywhere in W: every element of V and s is NaN, conv = (NaN, NaN), the call returns 0, and no index derived from data leaves
    [0, k) -- the eigen-solve is skipped on a non-finite Gram diagonal and the eigenvalue ranking is a total order (NaN first; its index property is
    proved on the CPU under ASan/UBSan, tests/test_rank_order_host.py).  The next clean call on the same scratch has the bits of a fresh one.
  * W finite, Vprev non-finite: s has the clean call's bits, every row of V is bitwise plus or minus the clean row, conv = (NaN, NaN).
  * batched launch: a bad sample changes no bit of any other sample's V, U, s or conv.
  * the loops of pullback.py raise DpbError on a non-finite conv and never count it as converged (tests/test_stop_rule_host.py on a stub; here
    on an fp16 engine whose cotangent overflows).
Every k of every eigen-solve and apply route is covered at N = 300 (R.NF_SHAPES), the grid-stride route once, both DPB_EIG_PAR routes in their child.
tests/test_orth_host.py holds the numpy restatement to the same assertions and keeps three mutants failing them: the plain-comparison ranking (slots
of `order` unwritten, s finite through them), the lam > 0 ? lam : 0 clamp (s == 0 beside a NaN V) and the NaN-dropping maximum (conv[1] == 0).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _norm_ref as NR
import _orth_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = lambda c: f"{c[0]}x{c[1]}-{c[2]}dec-{c[3]}"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------ (a) accuracy per route
@pytest.mark.parametrize("case", R.ACCURACY_CASES, ids=IDS)
def test_accuracy_per_route(case):
    k, N, decades, route = case
    c = R.case(k, N, decades)
    R.check(*R.gpu_orth(c.W, c.Vprev), c, k, N, decades, route)


@pytest.mark.parametrize("decades", R.BEYOND)
def test_beyond_the_pinned_domain_stays_finite(decades):
    """five and six decades (module docstring): finite, and the leading half of s exact; the rest is recorded"""
    k, N = R.LADDER_SHAPE
    c = R.case(k, N, decades)
    V, s, conv = R.gpu_orth(c.W, c.Vprev)
    m = R.measure(V, s, conv, c)
    print(R.line(k, N, decades, "beyond", m))
    assert np.isfinite(V).all() and np.isfinite(s).all() and np.isfinite(conv).all()
    assert m["s_ulps_rows"][:k // 2].max() <= 1.0


# ------------------------------------------------------------------------------------------------------------ (b) converged input
@pytest.mark.parametrize("k,N", R.CONVERGED)
def test_converged_input(k, N):
    """W = diag(sigma) Vprev: the Gram matrix is diagonal up to Vprev's own rounding, the solver's stop rule fires after one sweep, and the two
    convergence figures are checked at the magnitude at which the iteration's stop test reads them"""
    c = R.converged_case(k, N)
    m = R.check(*R.gpu_orth(c.W, c.Vprev), c, k, N, 2, "converged")
    assert m["dmax"] <= 1e-6


# ------------------------------------------------------------------------------------------------------------ (c) exact cases
@pytest.mark.parametrize("k", R.EXACT_K)
def test_ties_are_exact_and_keep_input_order(k):
    """one-hot rows: the Gram matrix is exactly diagonal, nothing rotates; descending sigma, ties in input order, every row once, all bits"""
    W, V_want, s_want, Vp = R.make_ties(k, 300)
    V, s, conv = R.gpu_orth(W, Vp)
    assert np.array_equal(V.sum(axis=0), V_want.sum(axis=0)), "a row is duplicated or missing"
    assert np.array_equal(V, V_want), (V.argmax(axis=1), V_want.argmax(axis=1))
    assert np.array_equal(s, s_want), (s, s_want)
    assert np.array_equal(conv, [0.0, 0.0]), conv


@pytest.mark.parametrize("k", R.EXACT_K)
def test_dead_direction_is_an_exact_zero_row(k):
    c = R.dead_case(k, 700)
    V, s, conv = R.gpu_orth(c.W_full, c.Vprev_full)
    assert not V[-1].any() and s[-1] == 0
    R.check(V, s, conv, c, k, 700, 2, "dead", Vprev=c.Vprev_full)


@pytest.mark.parametrize("k", R.EXACT_K)
def test_all_zero_input(k):
    _, Vp = R.make(k, 700, 2)
    V, s, conv = R.gpu_orth(np.zeros_like(Vp), Vp)
    assert not V.any() and not s.any()
    want = np.linalg.norm(Vp.astype(np.float64))
    assert abs(float(conv[0]) - want) <= R.U32 * want
    assert conv[1] == np.abs(Vp).max()


# ------------------------------------------------------------------------------------------------------------ (d) near rank deficiency
@pytest.mark.parametrize("k,N", R.DEFICIENT)
def test_near_rank_deficiency(k, N):
    """two rows are fp32 combinations of the others: everything finite, the leading k - 2 rows at the bounds; the two trailing s are rounding noise
    (module docstring) and only required finite and >= 0"""
    c = R.deficient_case(k, N)
    V, s, conv = R.gpu_orth(c.W, c.Vprev)
    assert np.isfinite(V).all() and np.isfinite(s).all() and (s >= 0).all() and np.isfinite(conv).all()
    print(f"k={k} N={N}: trailing s {s[-2:]} (leading {s[0]:.4f})")
    m = R.measure(V, s, conv, c)
    print(R.line(k, N, 2, "deficient", m))
    assert m["vec"] <= R.bounds(2)[0] and m["on"] <= R.bounds(2)[1] and m["s_ulps"] <= 1.0 and m["overlap"] >= -1e-9
    assert m["conv0_ulps"] <= 1.0 and m["conv1_err"] <= R.U32 * m["dmax"]


# ------------------------------------------------------------------------------------------------------------ (e) bitwise claims
@pytest.mark.parametrize("k,N", [(5, 1000), (50, 4099), (128, 65795)])
def test_repeatable_and_in_place_bits(k, N):
    """include/dpb.h: "bitwise reproducible", "V may alias Vprev" -- the loop of dpb_pullback_iterate calls it in place"""
    W, Vp = R.inputs(k, N, 2)
    Wd, Vpd = torch.from_numpy(W).to(DEV), torch.from_numpy(Vp).to(DEV)
    first = R.gpu_orth(Wd, Vpd)
    assert _same_bits(first, R.gpu_orth(Wd, Vpd)), "two calls differ"
    assert _same_bits(first, R.gpu_orth(Wd, Vpd, inplace=True)), "the in-place call differs"
    assert np.array_equal(Vpd.cpu().numpy(), Vp)                   # the out-of-place calls left Vprev alone


def _linear_tape():
    """one linear op, 16 -> 24 channels on 40 rows, fp32: N = 640, ragged against the 256-column slices"""
    g = torch.Generator().manual_seed(5)
    params = {"p.weight": torch.randn(24, 16, generator=g) / 4.0, "p.bias": 0.5 * torch.randn(24, generator=g)}
    return NR.build_tape([NR.linear("o", "x", "p", 24)], params, torch.float32, DEV, 40, 16)


NAN_BATCH = [(3, 3), (3, 20), (2, 128)]          # cyclic | round-robin in LDS | eigenvectors in global memory


@pytest.mark.parametrize("B,k", [(3, 3), (3, 12), (3, 20), (3, 60), (2, 128)])
def test_batched_launch_equals_single_launches(B, k):
    """dpb_pullback_iterate re-orthonormalises all samples in one set of launches (OrthArgs::batch, the sample on a grid axis), in place: one
    iteration must return the bits of Engine.orth on each sample's W = J^T J V0, and each sample meets the SVD bounds.  For NAN_BATCH the iteration
    is run once more with a row of sample 1's V0 set to NaN: sample 1 comes back all NaN in V and s with conv = (NaN, NaN), and V, U, s and conv of
    every other sample keep the bits of the clean run"""
    N = 640
    e = NR.engine(_linear_tape(), B, B * k)
    g = torch.Generator().manual_seed(100 + k)
    x = torch.randn(B, 40, 16, generator=g).to(DEV)
    rng = np.random.default_rng([k, B])
    V0 = np.concatenate([np.linalg.qr(rng.standard_normal((N, k)))[0].T for _ in range(B)])
    V0 = torch.from_numpy(np.ascontiguousarray(V0, dtype=np.float32)).to(DEV)
    e.primal(NR.to_nchw(x), 1.0, None, "o")
    W = e.vjp("o", e.jvp("o", V0)).clone()
    V, U, s, conv = e.iterate("o", V0.clone(), 1)
    torch.cuda.synchronize()
    for b in range(B):
        rows = slice(b * k, (b + 1) * k)
        single = [t.cpu().numpy() for t in e.orth(W[rows], V0[rows])]
        batched = (V[rows].cpu().numpy(), s[rows].cpu().numpy(), conv[b].cpu().numpy())
        c = R.Case(W[rows].cpu().numpy(), V0[rows].cpu().numpy())
        print(f"B={B} k={k} sample {b}: singular values of W over {c.sqrtS[0] ** 2 / c.sqrtS[-1] ** 2:.1f}x")
        R.check(*single, c, k, N, 2, f"batch{B}-single{b}")
        assert _same_bits(single, batched), f"sample {b}: the batched launch differs from the single one"
    if (B, k) in NAN_BATCH:
        clean = [t.cpu().numpy() for t in (V.view(B, k, N), U.view(B, k, -1), s.view(B, k), conv)]
        V0b = V0.clone()
        V0b[k + k // 2] = float("nan")                             # one row of sample 1
        got = e.iterate("o", V0b, 1)
        torch.cuda.synchronize()
        Vb, Ub, sb, cb = got[0].view(B, k, N).cpu().numpy(), got[1].view(B, k, -1).cpu().numpy(), got[2].view(B, k).cpu().numpy(), got[3].cpu().numpy()
        R.assert_all_nan(Vb[1], sb[1], cb[1], f"B={B} k={k}: the poisoned sample")
        for b in range(B):
            if b != 1:
                assert _same_bits((Vb[b], Ub[b], sb[b], cb[b]), (clean[0][b], clean[1][b], clean[2][b], clean[3][b])), \
                    f"B={B} k={k}: sample {b} changed because sample 1 held a NaN"
    del e


# ------------------------------------------------------------------------------------------------------------ (e2) non-finite input
@pytest.mark.parametrize("k,N", R.NF_SHAPES)
def test_non_finite_w_is_all_nan_and_leaves_no_state(k, N):
    """a NaN, +inf or -inf at W[0][0] or at W[k-1][N-1], or a whole row of NaN: V, s and conv are entirely NaN (exact: NaN masks), and the next call
    on clean data with the SAME scratch returns the bits of a clean call on a fresh scratch"""
    W, Vp = R.inputs(k, N, 2)
    Wd, Vpd = torch.tensor(W, device=DEV), torch.tensor(Vp, device=DEV)
    clean = R.gpu_orth(Wd, Vpd)
    assert all(np.isfinite(a).all() for a in clean)
    scratch = R.gpu_scratch(k, N, DEV)
    for how in R.NF_POISONS:
        R.assert_all_nan(*R.gpu_orth(R.poisoned(W, how), Vpd, scratch=scratch), f"k={k} N={N} {how}")
        assert _same_bits(clean, R.gpu_orth(Wd, Vpd, scratch=scratch)), f"k={k} N={N}: the clean call after {how} on the same scratch differs"


@pytest.mark.parametrize("k", R.NF_VPREV_K)
def test_non_finite_vprev_only_touches_signs_and_conv(k):
    """W finite, Vprev poisoned: s keeps the clean call's bits, every row of V is bitwise plus or minus the clean row, conv = (NaN, NaN)"""
    W, Vp = R.inputs(k, R.NF_N, 2)
    Wd = torch.tensor(W, device=DEV)
    clean = R.gpu_orth(Wd, Vp)
    for how in R.NF_POISONS:
        if how != "nan-row":
            R.assert_vprev_rule(R.gpu_orth(Wd, R.poisoned(Vp, how)), clean, f"k={k} Vprev {how}")


@pytest.mark.parametrize("k,how", [(5, "nan-tail"), (65, "pinf-first")])
def test_non_finite_w_in_place(k, how):
    W, Vp = R.inputs(k, R.NF_N, 2)
    R.assert_all_nan(*R.gpu_orth(R.poisoned(W, how), Vp, inplace=True), f"k={k} {how} in place")


def _fp16_overflow_net(B, k):
    """the smallest real engine, one fp16 linear op 16 -> 24 on 40 rows with weights of the order 8000: J^T J V passes 65504 in the fp16 cotangent,
    so dpb_orth is handed inf.  Returns a stand-in for the PullbackUNet the loops are methods of, around a real Engine."""
    import types
    g = torch.Generator().manual_seed(6)
    params = {"p.weight": (8192.0 * torch.randn(24, 16, generator=g)).clamp(-60000.0, 60000.0), "p.bias": torch.zeros(24)}
    tape = NR.build_tape([NR.linear("o", "x", "p", 24)], params, torch.float16, DEV, 40, 16)
    eng = NR.engine(tape, B, B * k)
    return types.SimpleNamespace(engine=eng, max_rank=B * k, device=DEV, verbose=False, k_shard_group=False, _tap=lambda op, block_idx: "o")


def test_fp16_overflow_raises_in_the_power_iterations():
    """the stop rule of pullback.py on a real engine: an fp16 tangent that overflows must end the loops with DpbError naming the iteration (and, in
    the batch form, the samples), not with a "converged" NaN basis"""
    from diffusion_pullback_amd import lib as L
    from diffusion_pullback_amd.pullback import PullbackUNet
    k = 3
    g = torch.Generator().manual_seed(7)
    V0 = torch.linalg.qr(torch.randn(640, k, generator=g))[0].T.contiguous()
    x = 1e-3 * torch.randn(2, 16, 40, 1, generator=g)
    net = _fp16_overflow_net(1, k)
    with pytest.raises(L.DpbError, match=r"iteration 0 are not finite"):
        PullbackUNet._pullback(net, x[:1], 1.0, None, None, None, k, 1, 1, 6, 1e-3, V0)
    del net
    net = _fp16_overflow_net(2, k)
    with pytest.raises(L.DpbError, match=r"iteration 0 are not finite for sample\(s\) \[0, 1\]"):
        PullbackUNet.local_encoder_pullback_batch(net, x, 1.0, None, None, None, pca_rank=k, min_iter=1, max_iter=6, convergence_threshold=1e-3, V0=V0)
    del net


# ------------------------------------------------------------------------------------------------------------ (f) the A/B solver routes
_CHILD = """
import sys
sys.path.insert(0, {tests!r})
import _orth_ref as R
for k in {ks!r}:
    c = R.case(k, 1000, 2)
    R.check(*R.gpu_orth(c.W, c.Vprev), c, k, 1000, 2, {route!r})
    R.assert_all_nan(*R.gpu_orth(R.poisoned(c.W, "nan-tail"), c.Vprev), (k, {route!r}))
    print("ORTH-NAN", k, {route!r})
"""


def test_solver_routes_behind_the_switch():
    """DPB_EIG_PAR is read once per process: 0 runs the one-wave cyclic solver wherever it exists (eig_kernel<16> at 6 and 16, eig_kernel<56> at 17
    and 56 -- reachable no other way), 2 the round-robin solver for k <= 5.  One fresh child per route, one after the other; the second starts only if
    the first returned 0, and a child that died on a signal or ran out of time ends the test at once."""
    for par, ks, route in (("0", [6, 16, 17, 56], "cyclic"), ("2", [1, 2, 5], "roundrobin")):
        env = dict(os.environ, PYTHONPATH=ROOT, DPB_EIG_PAR=par)
        code = _CHILD.format(tests=os.path.join(ROOT, "tests"), ks=ks, route=route)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
        print(r.stdout)
        if r.returncode < 0:
            pytest.fail(f"DPB_EIG_PAR={par}: the child died on signal {-r.returncode}; nothing more is started\n{r.stderr[-2000:]}", pytrace=False)
        assert r.returncode == 0, r.stderr[-3000:]
        assert r.stdout.count("ORTH-ERR") == len(ks)
        assert r.stdout.count("ORTH-NAN") == len(ks)              # and a NaN in W is all NaN out on the route (module docstring, non-finite input)


# ------------------------------------------------------------------------------------------------------------ (g) argument checks
def test_checked_entry_refuses_bad_arguments_and_writes_nothing():
    import ctypes as C

    from diffusion_pullback_amd import lib as L
    lib = L.load()
    k, N = 4, 300
    W, Vp = R.make(k, N, 2)
    Wd, Vpd = torch.from_numpy(W).to(DEV), torch.from_numpy(Vp).to(DEV)
    need = int(lib.dpb_orth_scratch_bytes(k, N))
    out = [torch.full((k, N), -7.0, device=DEV), torch.full((k,), -7.0, device=DEV), torch.full((2,), -7.0, device=DEV)]
    scratch = torch.zeros(need // 8 + 1, dtype=torch.float64, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda kk, nn, nbytes: lib.dpb_orth_checked(Wd.data_ptr(), Vpd.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                                       scratch.data_ptr(), nbytes, kk, nn, st)
    for kk, nn, nbytes, word in [(0, N, need, "k=0"), (129, N, 1 << 30, "k=129"), (k, 0, need, "N=0"), (k, N, need - 1, "scratch")]:
        assert call(kk, nn, nbytes) != 0, (kk, nn, nbytes)
        msg = lib.dpb_last_error().decode()
        assert word in msg, (word, msg)
        torch.cuda.synchronize()
        assert all(bool((t == -7.0).all()) for t in out), f"{word}: an output was written"
    assert lib.dpb_orth_scratch_bytes(0, N) == 0 and lib.dpb_orth_scratch_bytes(129, N) == 0 and lib.dpb_orth_scratch_bytes(k, 0) == 0
    assert call(k, N, need) == 0                                  # and the exact size is enough
    torch.cuda.synchronize()
    assert all(bool((t != -7.0).all()) for t in out)
