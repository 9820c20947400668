"""CPU checks of tests/_product_ref.py, the reference of tests/test_gpu_product_ops.py: the exact tier's adjoint identity and precondition for every
case, the real tier's bound against a plain fp32 evaluation (admitted) and against one whose K sum is carried in bf16 (rejected), the sinusoid
against the oracle's, and the GPU file's table of forced codes against what the library documents."""
import pytest
import torch

import _product_ref as R

F = torch.nn.functional
CASES = list(R.CASES.values())
DTYPES = [R.F32, R.BF, R.F16]


def _data(case, tier, dtype, B=2, kps=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    p = R.make_params(case, g, tier, dtype)
    x, V, U = R.make_inputs(case, g, tier, dtype, B, kps)
    ts = (0.0,) * B if tier == "exact" or not case.rowbias else tuple(case.t_real[:B])
    return p, x, V, U, ts


def test_table_holds_the_edges_it_names():
    c = R.CASES
    assert c["rows40_72_200"].cin % 64 == 8 and c["rows40_72_200"].cin % 32 == 8 and c["rows40_72_200"].steps[0]["cout"] % 64
    assert 600 % 32 == 24 and 600 % 128 == 88 and c["rows300_320_320"].hw[0] * 2 == 600
    assert c["rows264_328_264"].cin % 64 == 8 and c["rows264_328_264"].steps[0]["cout"] % 256 == 8
    assert c["rows24_8_13"].steps[0]["cout"] % 8
    assert c["c3_16x8_64_72"].hw[0] * c["c3_16x8_64_72"].hw[1] == 128 and c["c3_12x20_40_40"].cin % 64
    assert c["s2p1_16x12_72_136"].out_hw() == (8, 6) and c["s2p1_15x9_40_24"].out_hw() == (8, 5) and c["s2p0_16x12_40_72"].out_hw() == (8, 6)
    assert c["up_6x10_72_40"].out_hw() == (12, 20)
    assert c["two_6x10_24_40"].extra_roundings("adjoint") == 1 and c["two_6x10_24_40"].extra_roundings("primal") == 1
    assert c["rows40_72_200"].extra_roundings("primal") == 0 and c["rows40_72_200"].k_total("adjoint") == 200


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_exact_tier_adjoint_identity_and_precondition(case):
    """<U, J v> == <J^T U, v> exactly (integers in fp64), and the absolute-value sums stay below 2^24 (|ref| below 65504 for fp16)"""
    for B, kps in ((2, 2), (1, 1)):
        p, x, V, U, ts = _data(case, "exact", R.F16, B, kps)
        top = R.check_exact_precondition(case, p, x, V, U, R.F16, kps, ts)
        assert top < 2.0 ** 24
        O, dO, gX = R.reference(case, p, x, V, U, R.F16, kps, ts)
        assert float((U.double() * dO).sum()) == float((gX * V.double()).sum())
        assert dO.abs().max() > 0 and gX.abs().max() > 0
        for dt in DTYPES:                              # what the engine must return is a rounding of the integers, and a different one per dtype
            eO, edO, egX = R.exact_reference(case, p, x, V, U, dt, kps, ts)
            assert eO.dtype == torch.float32 and torch.equal(eO, eO.to(dt).float()) and torch.equal(egX, egX.to(dt).float())
            if dt == R.F32:
                assert torch.equal(eO.double(), O) and torch.equal(edO.double(), dO) and torch.equal(egX.double(), gX)


def test_exact_tier_exercises_the_rounding_at_long_k():
    """at K = 9 x 640 a tenth of the bf16 outputs need rounding, and fp32 matmul of such data is exact under two K orders"""
    g = torch.Generator().manual_seed(3)
    a, w = torch.randint(-3, 4, (64, 5760), generator=g).float(), torch.randint(-2, 3, (96, 5760), generator=g).float()
    ref = a.double() @ w.double().T
    assert float((a.abs() @ w.abs().T).max()) < 2.0 ** 24
    assert torch.equal((a @ w.T).double(), ref) and torch.equal((a.flip(1) @ w.flip(1).T).double(), ref)
    assert (ref.float().bfloat16().double() != ref).double().mean() > 0.05


def _fp32_eval(case, p, x, V, U, dtype, kps, ts, carry=None):
    """the three passes in plain fp32 (conv2d of the rounded inputs), rounded once to `dtype`.  carry: the K sum in chunks of 8 input channels with
    the running sum stored in that dtype after every chunk"""
    def net(xx, temb, linear):
        if carry is None:
            return R.evaluate(case, p, xx.float(), dtype, temb, linear=linear, store=dtype)
        acc = None
        for c0 in range(0, case.cin, 8):
            sub = R.Case(case.name, case.hw, min(8, case.cin - c0), [dict(s, res=None, rowbias=False) for s in case.steps[-1:]])
            ps = {k: (v[:, c0:c0 + 8] if k.endswith(".weight") and k.split(".")[0] not in ("rb", "rbpad") else v) for k, v in p.items()}
            part = R.evaluate(sub, ps, xx[:, c0:c0 + 8].float(), dtype, linear=True)
            acc = part if acc is None else acc + part
            acc = acc.to(carry).float()
        return acc
    B = x.shape[0]
    O = net(x, R.temb_rows(ts)[torch.arange(B)].float() if case.rowbias else None, False)
    dO = net(V, None, True)
    return R.rnd(O, dtype), R.rnd(dO, dtype)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_real_bound_admits_plain_fp32_evaluation(case, dtype):
    p, x, V, U, ts = _data(case, "real", dtype)
    ref = R.reference(case, p, x, V, U, dtype, 2, ts)
    S = R.magnitude(case, p, x, V, U, dtype, 2, ts)
    slack = R.temb_slack(case, p, dtype, ts, 2)
    got = _fp32_eval(case, p, x, V, U, dtype, 2, ts)
    worst = {}
    for w, g_, r, s in zip(("primal", "tangent"), got, ref, S):
        R.compare_real(g_, r, R.real_bound(case, w, r, s, dtype, slack), f"{case.name} {dtype} {w}", worst, w)
    # the adjoint: autograd of the fp32 net
    v = torch.zeros_like(V).requires_grad_(True)
    (gX,) = torch.autograd.grad(R.evaluate(case, p, v, dtype, linear=True), v, U)
    R.compare_real(R.rnd(gX, dtype), ref[2], R.real_bound(case, "adjoint", ref[2], S[2], dtype), f"{case.name} {dtype} adjoint", worst, "adjoint")
    assert 0 < max(worst.values()) <= 1.0, worst
    if dtype != R.F32 and case.extra_roundings("primal") == 0:
        assert worst["primal"] > 0.25, worst           # the one rounding nearly exhausts the bound: it has no slack to hide a second one in


@pytest.mark.parametrize("case", [c for c in CASES if len(c.steps) == 1 and c.cin >= 40], ids=lambda c: c.name)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_real_bound_rejects_a_k_sum_carried_in_bf16(case, dtype):
    p, x, V, U, ts = _data(case, "real", dtype)
    ref = R.reference(case, p, x, V, U, dtype, 2, ts)
    S = R.magnitude(case, p, x, V, U, dtype, 2, ts)
    _, dO = _fp32_eval(case, p, x, V, U, dtype, 2, ts, carry=torch.bfloat16)
    with pytest.raises(AssertionError, match="beyond the bound"):
        R.compare_real(dO, ref[1], R.real_bound(case, "tangent", ref[1], S[1], dtype), "planted")


def test_compare_exact_names_the_worst_element():
    want = torch.zeros(2, 3, 4, 5)
    got = want.clone()
    got[1, 2, 3, 4] = 1.0
    with pytest.raises(AssertionError, match=r"sample 1, y 3, x 4, channel 2"):
        R.compare_exact(got, want, "planted")
    R.compare_exact(want.clone(), want, "same")


def test_h_w_swap_in_the_reference_is_seen():
    """a reference that takes the image as W x H is a different map on a non-square case: the exact comparison of the two fails"""
    case = R.CASES["c3_12x20_40_40"]
    p, x, V, U, ts = _data(case, "exact", R.BF)
    O = R.evaluate(case, p, x.double(), R.BF)
    H, W = case.hw
    swapped = R.evaluate(case, p, x.double().reshape(2, case.cin, W, H), R.BF).reshape(O.shape)
    with pytest.raises(AssertionError, match="elements differ"):
        R.compare_exact(R.rnd(swapped, R.BF), R.rnd(O, R.BF), "swapped")


def test_sinusoid_is_the_oracles():
    from oracle.unet_ddpm import timestep_embedding
    ts = (0.0, 1.0, 2.5, 11.0)
    want = timestep_embedding(torch.tensor(ts), R.TEMB).double()
    assert torch.allclose(R.temb_rows(ts), want, rtol=0, atol=4e-6)
    z = R.temb_rows((0.0,))[0]
    assert torch.equal(z[:R.TEMB // 2], torch.zeros(R.TEMB // 2, dtype=torch.float64)) and torch.equal(z[R.TEMB // 2:], torch.ones(R.TEMB // 2, dtype=torch.float64))


def test_forced_codes_of_the_gpu_table_are_documented():
    """every forced code of tests/test_gpu_product_ops.py carries the profile kind tests/test_gpu_gemm_tiles.py lists for it (include/dpb.h) and,
    given a product its tile takes, dpb_debug_gemm_plan plans it as a tile of its family"""
    import ctypes as C
    import os
    import test_gpu_gemm_tiles as T
    import test_gpu_product_ops as G
    for code, kind in {**T.KIND_16BIT, 128: 1, 600: 5}.items():
        assert G.CODES[code][1] == kind, code
    assert sorted(G.CODES) == sorted({**T.KIND_16BIT, 128: 1, 600: 5})
    assert sorted(c for f, cs in G.FAMILY.items() for c in cs) == sorted([0] + list(G.CODES))
    from diffusion_pullback_amd import lib as L
    if not os.path.exists(os.path.join(os.path.dirname(L.__file__), "libdpb.so")):
        pytest.skip("libdpb.so is not built: the plan of each forced code cannot be asked for")
    lib = L.load()
    k, t, s = C.c_int(), C.c_int(), C.c_int()
    try:
        for code, (fam, kind, builds, cin64) in G.CODES.items():
            L.check(lib.dpb_debug_set(b"gemm_tile", code))
            q = (L.DPB_BF16, 256, 128, 576, 16, 64) if code == 600 else (L.DPB_BF16, 256, 320, 320, 0, 0)
            L.check(lib.dpb_debug_gemm_plan(*q, 0, 64 << 20, C.byref(k), C.byref(t), C.byref(s)))
            assert k.value == {"reg": int(code == 128), "halo": 3}.get(fam, 2), (code, k.value, t.value)
            assert t.value in (code, code - 1), (code, t.value)
    finally:
        L.check(lib.dpb_debug_set(b"gemm_tile", 0))
