"""CPU checks of tests/_norm_ref.py: the fp64 restatements against torch.nn.functional, their tangents and adjoints against central finite
differences and the <Jv, u> = <v, J^T u> identity, the interleave permutation, the kps mapping, the route rules, and the comparator on planted
errors (a wrong group, one wrong row, a missing accumulate) at the loosest bounds the GPU test uses."""

import math

import pytest
import torch

import _norm_ref as R

F = torch.nn.functional
F64 = torch.float64


def _nets():
    g = torch.Generator().manual_seed(0)
    p = {**R.norm_params(g, ["n", "m"], 64), "p.weight": torch.randn(64, 64, generator=g) / 8, "p.bias": torch.randn(64, generator=g)}
    return p, {
        "gn": [R.gn("o", "x", "n", 8, 1e-5, False)],
        "gn_silu": [R.gn("o", "x", "n", 8, 1e-5, True)],
        "ln": [R.ln("o", "x", "n")],
        "geglu": [R.geglu("o", "x", 0)],
        "two_consumers": [R.gn("a", "x", "n", 8, 1e-5, True), R.gn("b", "x", "m", 8, 1e-5, True), R.concat("o", "a", "b")],
        "product_res_gn": [R.linear("r", "x", "p", 64), R.linear("c", "x", "p", 64, res="r"), R.gn("o", "c", "n", 8, 1e-5, True)],
    }


def test_restatements_match_torch_functional_in_fp64():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, 10, 64, generator=g, dtype=F64) * 2 + 1
    ga, be = [t.double() for t in R.affine(g, 64)]
    for G in (1, 8, 64):
        want = F.group_norm(x.permute(0, 2, 1), G, ga, be, 1e-5).permute(0, 2, 1)
        assert torch.allclose(R.group_norm_ref(x, ga, be, G, 1e-5), want, rtol=1e-12, atol=1e-12)
        assert torch.allclose(R.group_norm_ref(x, ga, be, G, 1e-5, True), F.silu(want), rtol=1e-12, atol=1e-12)
    assert torch.allclose(R.layer_norm_ref(x, ga, be, 1e-5), F.layer_norm(x, (64,), ga, be, 1e-5), rtol=1e-12, atol=1e-12)
    assert torch.allclose(R.gelu_erf(x), F.gelu(x), rtol=1e-13, atol=1e-13)
    assert torch.allclose(R.geglu_ref(x), x[..., :32] * F.gelu(x[..., 32:]), rtol=1e-13, atol=1e-13)
    ev = lambda fn: R.evaluate([R.unary("o", "x", fn)], {}, x, torch.float32)
    assert torch.allclose(ev("silu"), F.silu(x), rtol=1e-13) and torch.allclose(ev("gelu"), F.gelu(x), rtol=1e-13, atol=1e-13)
    assert torch.allclose(ev("quick_gelu"), x * torch.sigmoid(1.702 * x), rtol=1e-13)


@pytest.mark.parametrize("name", ["gn", "gn_silu", "ln", "geglu", "two_consumers", "product_res_gn"])
def test_reference_tangent_and_adjoint(name):
    """central finite differences (fp64, h = 1e-6: truncation ~1e-12 |f'''|, rounding ~1e-10) and the adjoint identity; tangent j uses sample j // kps"""
    params, nets = _nets()
    steps = nets[name]
    g = torch.Generator().manual_seed(2)
    B, kps, rows = 2, 2, 6
    x = torch.randn(B, rows, 64, generator=g)
    V = torch.randn(B * kps, rows, 64, generator=g)
    O, dO, _ = R.reference(steps, params, x, torch.float32, V, None, kps)
    U = torch.randn(B * kps, rows, O.shape[-1], generator=g)
    _, _, gX = R.reference(steps, params, x, torch.float32, None, U, kps)
    f = lambda xx: R.evaluate(steps, params, xx, torch.float32)
    h = 1e-6
    for j in range(B * kps):
        xs = x[j // kps:j // kps + 1].double()
        fd = (f(xs + h * V[j:j + 1].double()) - f(xs - h * V[j:j + 1].double())) / (2 * h)
        assert (fd - dO[j:j + 1]).norm() <= 1e-7 * dO[j].norm(), (name, j)
        wrong = x[1 - j // kps:2 - j // kps].double()                       # the other sample: a wrong j / kps mapping is visible
        fdw = (f(wrong + h * V[j:j + 1].double()) - f(wrong - h * V[j:j + 1].double())) / (2 * h)
        assert (fdw - dO[j:j + 1]).norm() >= 1e-2 * dO[j].norm(), (name, j)
    lhs = (dO * U.double()).sum((1, 2))
    rhs = (V.double() * gX).sum((1, 2))
    assert torch.allclose(lhs, rhs, rtol=1e-10, atol=1e-10), (name, lhs, rhs)


def test_interleave_permutation_is_the_tape_weight_permutation():
    """a product with interleave = 64 followed by geglu(il = 64) equals the split product followed by geglu(il = 0)"""
    from diffusion_pullback_amd.tape import Tape
    Fh = 128
    perm = R.interleave_perm(Fh, 64)
    assert perm[:64].tolist() == list(range(64)) and perm[64:128].tolist() == list(range(128, 192)) and perm[128:192].tolist() == list(range(64, 128))
    g = torch.Generator().manual_seed(3)
    w = torch.randn(2 * Fh, 16, generator=g)
    t = Tape({"p.weight": w}, torch.float32, "cpu")
    t._conv_w("p", 16, 2 * Fh, False, 64)
    assert torch.equal(t.keep[0], w[perm])                               # rows of the weight = columns of the product's output
    x = torch.randn(2, 5, 2 * Fh, generator=g, dtype=F64)
    assert torch.equal(R.geglu_ref(x[..., perm], 64), R.geglu_ref(x, 0))


def test_route_rules_restate_norm_hip():
    BF, F32 = torch.bfloat16, torch.float32
    assert R.gn_fused_groups(320, 32, 408, BF) == 4 and R.gn_fused_groups(320, 32, 409, BF) == 0
    assert R.gn_fused_groups(320, 32, 408, F32) == 2 and R.gn_fused_groups(1920, 32, 136, BF) == 2 and R.gn_fused_groups(1920, 32, 136, F32) == 1
    assert R.gn_fused_groups(2560, 32, 204, BF) == 1 and R.gn_fused_groups(2560, 32, 205, BF) == 0 and R.gn_fused_groups(2560, 32, 204, F32) == 0
    assert R.gn_fused_groups(128, 32, 72, BF) == 0 and R.gn_fused_groups(32, 32, 72, F32) == 0
    assert R.gn_route(32, 32, 2048, BF, 1) == ("red", 2) and R.gn_route(32, 32, 2056, BF, 1) == ("reduce", 3)
    assert R.gn_route(32, 32, 2056, BF, 4) == ("red", 2)
    assert R.gn_route(320, 32, 409, BF, 1, det=False, primal=True) == ("atomic", 3) and R.gn_route(320, 32, 409, BF, 2, False, False) == ("atomic", 2)
    assert R.ln_route(2048, BF) == "wave5" and R.ln_route(1536, BF) == "wave3" and R.ln_route(768, BF) == "rows32x3" and R.ln_route(768, F32) == "wave3"


def _loosest(families, which):
    """the loosest row bound the GPU test uses for these families (over dtypes)"""
    return max(R.BOUNDS[(f, d)][which][0] for f in families for d in (torch.float32, torch.bfloat16, torch.float16) if (f, d) in R.BOUNDS)


def test_comparator_catches_planted_errors_at_the_gpu_bounds():
    params, nets = _nets()
    g = torch.Generator().manual_seed(4)
    B, kps, rows, G = 2, 2, 24, 8
    x = torch.randn(B, rows, 64, generator=g)
    V = torch.randn(B * kps, rows, 64, generator=g)
    U = torch.randn(B * kps, rows, 64, generator=g)
    O, dO, gX = R.reference(nets["gn_silu"], params, x, torch.float32, V, U, kps)
    gn_bound = _loosest(("gn_fused", "gn_two_pass", "gn_atomic", "acc_gn"), "primal")
    assert R.errors(O, O, G)[0] == 0.0
    # a wrong group: group 3 of sample 1 normalised with the statistics of group 4
    xg = x.double().reshape(B, rows, G, 8)
    mean, var = xg.mean((1, 3), keepdim=True), xg.var((1, 3), keepdim=True, unbiased=False)
    mean[1, :, 3], var[1, :, 3] = mean[1, :, 4], var[1, :, 4]
    y = ((xg - mean) / torch.sqrt(var + 1e-5)).reshape(B, rows, 64) * params["n.weight"].double() + params["n.bias"].double()
    bad = y * torch.sigmoid(y)
    e = R.row_errors(bad, O, G)
    assert e[1, 3] > gn_bound and float(e.max()) == float(e[1, 3])
    e[1, 3] = 0
    assert e.max() < 1e-12                                              # every other (sample, group) is untouched
    with pytest.raises(AssertionError, match="group 3"):
        R.compare(bad, O, G, gn_bound, math.inf, "primal planted")
    # the same error seen per token row is spread over all rows: it still shows, the group view names it
    assert R.errors(bad, O, 0)[0] > gn_bound
    # one wrong row (LayerNorm view): row 5 of tangent 2 is the row of the wrong sample
    Ol, dOl, _ = R.reference(nets["ln"], params, x, torch.float32, V, None, kps)
    _, dOw, _ = R.reference(nets["ln"], params, x.flip(0), torch.float32, V, None, kps)
    badl = dOl.clone()
    badl[2, 5] = dOw[2, 5]
    ln_bound = _loosest(("ln", "acc_ln", "slab_ln", "geglu", "concat"), "tangent")
    with pytest.raises(AssertionError, match=r"tangent 2, row 5"):
        R.compare(badl, dOl, 0, ln_bound, math.inf, "tangent planted")
    # a wrong j / kps mapping: tangent 1 computed on sample 1 instead of sample 0
    badk = dO.clone()
    badk[1] = R.reference(nets["gn_silu"], params, x[1:], torch.float32, V[1:2], None, 1)[1][0]
    assert R.errors(badk, dO, G)[0] > _loosest(("gn_fused", "gn_two_pass", "gn_atomic"), "tangent")
    # a missing accumulate: the cotangent of x holds one consumer's contribution only
    steps = nets["two_consumers"]
    U2 = torch.randn(B * kps, rows, 128, generator=g)
    _, _, gfull = R.reference(steps, params, x, torch.float32, None, U2, kps)
    _, _, gone = R.reference([steps[1]], params, x, torch.float32, None, U2[..., 64:], kps)
    acc_bound = _loosest(("acc_gn", "acc_ln"), "adjoint")
    with pytest.raises(AssertionError):
        R.compare(gone, gfull, G, acc_bound, math.inf, "adjoint planted")
    assert R.row_errors(gone, gfull, G).min() > acc_bound                # every group misses a contribution


def test_bounds_are_not_surprising():
    """primal bounds stay within 2 x 16 unit roundoffs of the dtype on the zero-mean families (a larger measured error is a finding, not a bound)"""
    for (fam, dtype), b in R.BOUNDS.items():
        if fam in ("gn_fused", "gn_two_pass", "ln", "geglu", "unary"):
            assert b["primal"][0] <= 32 * R.UNIT[dtype], (fam, dtype, b)


def test_ladder_inputs_have_the_means_they_claim():
    g = torch.Generator().manual_seed(5)
    x = R.ladder_input(g, 2, 50, 64, torch.float32, 64.0, 0.25, groups=8).reshape(2, 50, 8, 8)
    m = x.mean((1, 3))
    assert ((m.abs() - 64).abs() < 0.1).all() and (x.std((1, 3)) < 0.3).all() and (m > 0).any() and (m < 0).any()
    r = R.ladder_input(g, 2, 50, 64, torch.float32, 256.0, 0.25)
    assert ((r.mean(-1).abs() - 256).abs() < 0.2).all()
    assert len(R.ladder_rungs(torch.bfloat16)) == 2 and len(R.ladder_rungs(torch.float16)) == 3 and len(R.ladder_rungs(torch.float32)) == 4


def test_torch_norms_differentiate_in_forward_mode():
    """the ladder's yardstick: torch.func.jvp through group_norm / layer_norm"""
    g = torch.Generator().manual_seed(6)
    x, v = torch.randn(1, 12, 64, generator=g), torch.randn(1, 12, 64, generator=g)
    ga, be = R.affine(g, 64)
    _, d = torch.func.jvp(lambda a: F.group_norm(a.permute(0, 2, 1), 8, ga, be, 1e-5).permute(0, 2, 1), (x,), (v,))
    ref = R.reference([R.gn("o", "x", "n", 8)], {"n.weight": ga, "n.bias": be}, x, torch.float32, v, None, 1)[1]
    assert R.errors(d, ref, 8)[0] < 1e-5
    _, d = torch.func.jvp(lambda a: F.layer_norm(a, (64,), ga, be, 1e-5), (x,), (v,))
    ref = R.reference([R.ln("o", "x", "n")], {"n.weight": ga, "n.bias": be}, x, torch.float32, v, None, 1)[1]
    assert R.errors(d, ref, 0)[0] < 1e-5
