"""CPU checks of the op-level attention test kit (tests/_attn_ref.py): the crafted score patterns realise the growth sequences they claim after
16-bit rounding, the fp64 autograd reference agrees with the closed forms, and the per-row comparator catches local corruptions at the bounds
the GPU tests use."""
import math

import pytest
import torch

import _attn_ref as R

F16S = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float16, id="fp16")]


@pytest.mark.parametrize("dtype", F16S)
@pytest.mark.parametrize("d", [40, 64, 80, 160])
def test_patterns_realise_their_growth_sequences(dtype, d):
    for L in ((256, 1024) if d != 160 else (64, 256)):
        for p in R.PATTERNS:
            Q, K, _ = R.crafted_qkv(p, L, 2, d, dtype)
            R.check_pattern(p, Q, K, d, 2)


def test_pattern_checker_rejects_a_wrong_claim():
    Q, K, _ = R.crafted_qkv("P2", 1024, 1, 40, torch.bfloat16)
    with pytest.raises(AssertionError):
        R.check_pattern("P3", Q, K, 40, 1)                    # 3.9 log2 units never cross the threshold
    Q, K, _ = R.crafted_qkv("P3", 1024, 1, 40, torch.bfloat16)
    with pytest.raises(AssertionError):
        R.check_pattern("P2", Q, K, 40, 1)


def _tiny(B=2, L=12, H=2, d=8, kps=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    C = H * d
    x = torch.randn(B, L, 3 * C, generator=g, dtype=torch.float64)
    V = torch.randn(B * kps, L, 3 * C, generator=g, dtype=torch.float64)
    U = torch.randn(B * kps, L, C, generator=g, dtype=torch.float64)
    return x, V, U, C


def test_reference_agrees_with_closed_form_jvp_and_vjp():
    B, L, H, d, kps = 2, 12, 2, 8, 2
    x, V, U, C = _tiny(B, L, H, d, kps)
    O, dO, gX = R.reference(x, H, d, (0, C, 2 * C), V, U, kps=kps)
    for j in range(B * kps):
        b = j // kps
        for h in range(H):
            s = slice(h * d, (h + 1) * d)
            win = lambda t, w: t[:, w * C:(w + 1) * C][:, s]
            o, do, (gq, gk, gv) = R.closed_form(win(x[b], 0), win(x[b], 1), win(x[b], 2), win(V[j], 0), win(V[j], 1), win(V[j], 2), U[j, :, s],
                                                1 / math.sqrt(d))
            torch.testing.assert_close(O[b, :, s], o)
            torch.testing.assert_close(dO[j, :, s], do)
            torch.testing.assert_close(win(gX[j], 0), gq)
            torch.testing.assert_close(win(gX[j], 1), gk)
            torch.testing.assert_close(win(gX[j], 2), gv)


def test_reference_aliased_cross_and_causal_forms():
    B, L, H, d, kps = 2, 12, 2, 8, 2
    x, V, U, C = _tiny(B, L, H, d, kps, seed=1)
    x1, V1 = x[..., :C], V[..., :C]
    # aliased: q = k = v = x1 -- the same as the three-window op on [x1 | x1 | x1] with the window gradients summed
    Oa, dOa, gXa = R.reference(x1, H, d, (0, 0, 0), V1, U, kps=kps)
    O3, dO3, gX3 = R.reference(x1.repeat(1, 1, 3), H, d, (0, C, 2 * C), V1.repeat(1, 1, 3), U, kps=kps)
    torch.testing.assert_close(Oa, O3)
    torch.testing.assert_close(dOa, dO3)
    torch.testing.assert_close(gXa, gX3[..., :C] + gX3[..., C:2 * C] + gX3[..., 2 * C:])
    # cross: constant K / V of a context -> the tangent ignores the context, the adjoint is gQ alone
    ctx = x[:, :7, C:]
    Oc, dOc, gXc = R.reference(x1, H, d, (0, 0, C), V1, U, kps=kps, ctx=ctx)
    for j in range(B * kps):
        b = j // kps
        for h in range(H):
            s = slice(h * d, (h + 1) * d)
            z = torch.zeros(7, d, dtype=torch.float64)
            o, do, (gq, _, _) = R.closed_form(x1[b, :, s], ctx[b, :, s], ctx[b, :, C:][:, s], V1[j, :, s], z, z, U[j, :, s], 1 / math.sqrt(d))
            torch.testing.assert_close(Oc[b, :, s], o)
            torch.testing.assert_close(dOc[j, :, s], do)
            torch.testing.assert_close(gXc[j, :, s], gq)
    # causal: row i equals the full attention over the first i + 1 keys
    Ok = R.reference(x, H, d, (0, C, 2 * C), causal=True)[0]
    for i in (0, 5, L - 1):
        torch.testing.assert_close(Ok[:, i], R.reference(x[:, :i + 1], H, d, (0, C, 2 * C))[0][:, i])


# ------------------------------------------------------------------------------------------------ comparator sensitivity
FAMILIES = [pytest.param(k, id=f"{k[0]}-{str(k[1])[6:]}") for k in R.BOUNDS]


def _case(seed=3, B=2, L=64, H=4, d=40, kps=2):
    x, V, U, C = _tiny(B, L, H, d, kps, seed)
    x = x * 2.0                                               # scores of a few units: peaked rows next to flat ones
    return R.reference(x, H, d, (0, C, 2 * C), V, U, kps=kps), x, V, U, C, H, d, kps


def _fails(out, ref, d, bounds):
    try:
        R.compare(out, ref, d, *bounds)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("family", FAMILIES)
def test_comparator_passes_a_copy_and_catches_a_scaled_row(family):
    (O, dO, gX), *_, d, kps = _case()
    # 2^-6 where the 16-bit format allows it; bf16's own rounding puts its row bounds at 0.8e-2 - 3.9e-2: 2^-4 there
    eps = 2 ** -4 if family[1] == torch.bfloat16 else 2 ** -6
    for name, ref in (("primal", O), ("tangent", dO), ("adjoint", gX)):
        b = R.BOUNDS[family][name]
        assert not _fails(ref.clone(), ref, d, b)
        if family[1] != torch.float32:                        # the engine's own output rounding alone must pass
            assert not _fails(ref.to(family[1]).double(), ref, d, b), name
        rn = ref.reshape(ref.shape[0], ref.shape[1], -1, d).norm(dim=-1)
        t, r, g = [int(i) for i in torch.unravel_index(rn.argmax(), rn.shape)]
        bad = ref.clone()
        bad[t, r, g * d:(g + 1) * d] *= 1 + eps                # one row of one head (the largest: the bound is relative to it)
        assert _fails(bad, ref, d, b), (name, family)


@pytest.mark.parametrize("family", FAMILIES)
def test_comparator_catches_swapped_heads(family):
    (O, dO, gX), *_, d, kps = _case()
    for name, ref in (("primal", O), ("tangent", dO), ("adjoint", gX)):
        bad = ref.clone()
        bad[..., 0:d], bad[..., d:2 * d] = ref[..., d:2 * d], ref[..., 0:d]
        assert _fails(bad, ref, d, R.BOUNDS[family][name]), (name, family)


@pytest.mark.parametrize("family", FAMILIES)
def test_comparator_catches_another_samples_softmax(family):
    (O, dO, gX), x, V, U, C, H, d, kps = _case()
    xm = x.clone()
    xm[1, :, :2 * C] = x[0, :, :2 * C]                        # sample 1 with sample 0's Q and K: sample 0's probabilities
    _, dOm, gXm = R.reference(xm, H, d, (0, C, 2 * C), V, U, kps=kps)
    for name, ref, mixed in (("tangent", dO, dOm), ("adjoint", gX, gXm)):
        bad = ref.clone()
        bad[kps:] = mixed[kps:]
        assert _fails(bad, ref, d, R.BOUNDS[family][name]), (name, family)


@pytest.mark.parametrize("family", FAMILIES)
def test_comparator_catches_a_dropped_aliased_cotangent(family):
    _, x, V, U, C, H, d, kps = _case()
    x1 = x[..., :C] / 2                                       # N(0, 1) as in the GPU test: the three cotangents of comparable size
    _, _, g3 = R.reference(x1.repeat(1, 1, 3), H, d, (0, C, 2 * C), None, U, kps=kps)
    parts = [g3[..., w * C:(w + 1) * C] for w in range(3)]
    ref = parts[0] + parts[1] + parts[2]
    for w in range(3):
        assert _fails(ref - parts[w], ref, d, R.BOUNDS[family]["adjoint"]), (w, family)
