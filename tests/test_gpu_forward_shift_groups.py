"""dpb_forward_shift_groups (Engine.forward_shift_groups): the grouped shared prefix -- `groups` shifted copies of xbatch DIFFERENT samples, the part of
the net up to the tap run once at xbatch -- on the nets, taps, directions and CPU restatement of tests/test_gpu_hshift.py.

Bars, those of that file: atol 1e-5 / rtol 1e-4 against the per-row call on the same engine (dpb_forward_shift with xbatch = batch, x repeated), rel
< 2e-4 against the fp32 CPU restatement of get_h_to_e at h_b + s u_d.  groups = 1 and xbatch = 1 are the existing calls bit for bit."""
import pytest
import torch

import test_gpu_hshift as HS
from _util import rel

pytestmark = pytest.mark.gpu
SHAPES = [(2, 2), (2, 3), (3, 2)]                   # (xbatch, groups)
ROW_DIRS, ROW_SCALES = [-1, 0, 1, 0, 1, -1], [0.0, 0.5, -2.0, 1.5, 0.7, 0.0]


def _x(S, xb):
    """xb samples: the two of the shared setup, the first again as a third (its ctx row with it)"""
    idx = [0, 1, 0][:xb]
    return S["x"][idx], None if S["ctx"] is None else S["ctx"][idx], idx


@pytest.mark.parametrize("xb,groups", SHAPES)
@pytest.mark.parametrize("kind", ["sd", "ddpm"])
def test_groups_vs_per_row_call_and_restatement(kind, xb, groups):
    S = HS._setup(kind)
    e = HS._net(kind, max_batch=6).engine
    t = float(S["t"])
    x, ctx, idx = _x(S, xb)
    B = xb * groups
    dirs, scales = ROW_DIRS[:B], ROW_SCALES[:B]
    errs = {}
    for tap in HS.TAPS[kind]:
        out = e.forward_shift_groups(x, groups, t, ctx, tap, S["u"][tap], dirs, scales).cpu()
        assert out.shape[0] == B
        rep = e.forward_shift(x.repeat(groups, 1, 1, 1), t, None if ctx is None else ctx.repeat(groups, 1, 1), tap, S["u"][tap], dirs, scales).cpu()
        assert torch.allclose(out, rep, atol=1e-5, rtol=1e-4), (tap, (out - rep).abs().max())
        errs[tap] = [rel(out[r:r + 1], HS._ref(kind, tap, idx[r % xb], dirs[r], scales[r] if dirs[r] >= 0 else 0.0)) for r in range(B)]
    print(kind, xb, groups, {k: max(v) for k, v in errs.items()})
    assert all(max(v) < 2e-4 for v in errs.values()), errs


@pytest.mark.parametrize("kind", ["sd", "ddpm"])
def test_groups_1_and_xbatch_1_are_the_existing_calls_bitwise(kind):
    S = HS._setup(kind)
    e = HS._net(kind, max_batch=4).engine
    t = float(S["t"])
    for tap in HS.TAPS[kind]:
        u = S["u"][tap]
        a = e.forward_shift_groups(S["x"], 1, t, S["ctx"], tap, u, [1, -1], [0.7, 0.0])
        assert torch.equal(a, e.forward_shift(S["x"], t, S["ctx"], tap, u, [1, -1], [0.7, 0.0])), tap
        x1, c1 = S["x"][0:1], HS._ctx(S, slice(0, 1))
        b = e.forward_shift_groups(x1, 4, t, c1, tap, u, HS.DIRS, HS.SCALES)
        assert torch.equal(b, e.forward_shift(x1, t, c1, tap, u, HS.DIRS, HS.SCALES)), tap


@pytest.mark.parametrize("kind", ["sd", "ddpm"])
def test_flops_are_the_prefix_once_and_the_rest_at_the_whole_batch(kind):
    """F(tap, b): gemm_flops after forward to tap at batch b.  The grouped call costs F(src, xbatch) + F(eps, B) - F(src, B), exactly (the identity of
    tests/test_gpu_hshift.py with xbatch in place of 1)."""
    S = HS._setup(kind)
    xb, groups = 2, 3
    B = xb * groups
    e = HS._net(kind, max_batch=B).engine
    t = float(S["t"])
    x, ctx, _ = _x(S, xb)
    xB, cB = x.repeat(groups, 1, 1, 1), None if ctx is None else ctx.repeat(groups, 1, 1)

    def flops(xx, cc, tap):
        e.forward(xx, t, cc, tap)
        return e.stats()[1]
    fE = flops(xB, cB, "eps")
    for tap in HS.TAPS[kind]:
        fx, fB = flops(x, ctx, tap), flops(xB, cB, tap)
        e.forward_shift_groups(x, groups, t, ctx, tap, S["u"][tap], ROW_DIRS, ROW_SCALES)
        fl = e.stats()[1]
        want = fx + fE - fB
        print(kind, tap, "flops", fl, "of", fE)
        assert fl < fE and abs(fl - want) <= 1e-9 * want, (tap, fl, want, fE)


def test_refusals_and_the_next_call():
    from diffusion_pullback_amd import DpbError
    S = HS._setup("sd")
    e = HS._net("sd", max_batch=4).engine
    t, tap = float(S["t"]), ("mid", 0)
    u = S["u"][tap]
    x, ctx = S["x"], S["ctx"]
    with pytest.raises(DpbError, match="above max_batch=4"):
        e.forward_shift_groups(x, 3, t, ctx, tap, u, [0] * 6, [1.0] * 6)
    with pytest.raises(DpbError, match="groups=0"):
        e.forward_shift_groups(x, 0, t, ctx, tap, u, [], [])
    for bad in ([0, 1, 2, 0], [0, -2, 0, 0]):
        with pytest.raises(DpbError, match="outside"):
            e.forward_shift_groups(x, 2, t, ctx, tap, u, bad, [1.0] * 4)
    with pytest.raises(DpbError, match="not finite"):
        e.forward_shift_groups(x, 2, t, ctx, tap, u, [0] * 4, [1.0, float("nan"), 1.0, 1.0])
    with pytest.raises(DpbError):                                        # no direction at all
        e.forward_shift_groups(x, 2, t, ctx, tap, u[:0], [0] * 4, [1.0] * 4)
    with pytest.raises(DpbError, match="not downstream"):
        e.forward_shift_groups(x, 2, t, ctx, tap, u, [0] * 4, [1.0] * 4, dst=("down", 0))
    with pytest.raises(DpbError, match="xbatch=2"):                      # dpb_forward_shift keeps its own contract
        e.forward_shift(x, t, ctx, tap, u, [0, 1, 0], [1.0] * 3)
    dirs, scales = [0, -1, 1, 0], [0.5, 0.0, -2.0, 1.5]
    a = e.forward_shift_groups(x, 2, t, ctx, tap, u, dirs, scales)
    b = e.forward_shift_groups(x, 2, t, ctx, tap, u, dirs, scales)
    assert torch.equal(a, b) and torch.isfinite(a).all()
    with pytest.raises(DpbError):                                        # no stash was kept: a jvp right after the call is refused
        e.jvp(tap, torch.zeros(1, e.n_in, device=HS.DEV))
