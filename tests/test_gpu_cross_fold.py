"""The folded route of the text-conditioned attention layers (dpb_debug_set("cross_fold", v), csrc/engine.cpp fold_route): the sample's constant
K / V multiplied into to_q / to_out once per sample, LayerNorm' -> to_q -> attention -> to_out as two products with the softmax Jacobian as the
epilogue of the first (EPI_XATT, csrc/epilogue.h).

Nets: one-block SD configs built up to the mid tap -- sample_size 8 (64 query rows), 77 context rows of width 768, 8 heads, one transformer
(mid_block.attentions.0), C = 640 and 1280 under the rule, C = 320 with cross_fold = 2, bf16 and fp16.  The passes run BETWEEN the input of the
layer's LayerNorm (norm2) and the output of attn2.to_out, so what is measured is the layer chain and nothing else.

Yardstick: an fp64 CPU restatement of that chain (LayerNorm -> to_q -> softmax attention on the stored K / V, head by head with
tests/_attn_ref._attend -> to_out + residual) at the primal values the engine holds (read back) and the weights rounded to the engine dtype,
differentiated by autograd.  The fold moves 16-bit roundings (Gt / Gk / F / Fk are rounded instead of the q tangent and the attention output) and
changes no formula, so the bar is the one tests/test_gpu_hshift.py uses for a moved rounding point: the folded route's error against fp64 is at
most 1.5 x the one-launch route's error on the same stash and inputs.  Both errors are printed.
"""
import ctypes as C
import functools

import pytest
import torch

from _attn_ref import _attend
from _util import rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HEADS, ROWS, SIDE, KEYS = 8, 64, 8, 77
TB = "mid_block.attentions.0.transformer_blocks.0"
DTYPES = [torch.bfloat16, torch.float16]
CASES = [(640, 1), (1280, 1), (320, 2)]              # (C, cross_fold value that selects the route there)


def _lib():
    from diffusion_pullback_amd import lib as L
    return L, L.load()


def _set(v):
    L, l = _lib()
    L.check(l.dpb_debug_set(b"cross_fold", int(v)))


@pytest.fixture(autouse=True)
def _default_switch():
    yield
    _set(1)


@functools.lru_cache(maxsize=None)
def _params(C_, heads):
    from oracle import unet_sd
    cfg = unet_sd.SDConfig(block_out_channels=(C_,), layers_per_block=1, down_attn=(False,), up_attn=(False,), heads=(heads,), cross_dim=768,
                           sample_size=SIDE, ctx_len=KEYS)
    g = torch.Generator().manual_seed(100 + C_ + heads)
    return cfg, unet_sd.init_params(cfg, seed=3), torch.randn(2, 4, SIDE, SIDE, generator=g), torch.randn(2, KEYS, 768, generator=g)


@functools.lru_cache(maxsize=None)
def _net(C_, dtype, heads=HEADS, max_batch=1):
    """the engine with three extra taps: "in" (input of norm2), "out" (output of attn2.to_out), "kv" (the context's K | V projection)"""
    from diffusion_pullback_amd import PullbackUNet
    cfg, p, _, _ = _params(C_, heads)
    net = PullbackUNet("sd", cfg, p, dtype=dtype, device=DEV, max_batch=max_batch, max_rank=5 * max_batch, upto=("mid", 0), verbose=False)
    t = net.engine.tape
    L, _ = _lib()
    ai = [i for i, o in enumerate(t.ops) if o["kind"] == L.OP_ATTENTION and o["in1"] != o["in0"]]
    assert len(ai) == 1
    a, q, o = t.ops[ai[0]], t.ops[ai[0] - 1], t.ops[ai[0] + 1]
    ln = [x for x in t.ops if x["out"] == q["in0"]][0]
    assert ln["kind"] == L.OP_LAYERNORM and o["res"] == ln["in0"] and q["out"] == a["in0"] and o["in0"] == a["out"]
    t.tap("in", ln["in0"], C_, SIDE, SIDE)
    t.tap("out", o["out"], C_, SIDE, SIDE)
    t.tap("kv", a["in1"], t.buffers[a["in1"]][1], KEYS, 1)
    return net, dict(op=ai[0], ok=a["ip"][2], ov=a["ip"][3])


def _run_primal(C_, dtype, heads=HEADS, batch=1, max_batch=1):
    net, info = _net(C_, dtype, heads, max_batch)
    _, _, x, ctx = _params(C_, heads)
    net.engine.primal(x[:batch], 500.0, ctx[:batch], ("mid", 0))
    return net, info


def _rows(t, n, C_):
    """NCHW-flattened [n, C * rows] -> [n, rows, C]"""
    return t.reshape(n, C_, ROWS).permute(0, 2, 1)


def _flat(t):
    """[n, rows, C] -> NCHW-flattened [n, C * rows]"""
    return t.permute(0, 2, 1).reshape(t.shape[0], -1).contiguous()


def _chain(C_, dtype, e, info, heads=HEADS):
    """fp64 restatement of norm2 -> attn2 (to_q, attention on the stored K / V, to_out) + residual at the engine's primal state: h -> out"""
    _, p, _, _ = _params(C_, heads)
    w = lambda n: p[n].detach().to(dtype).double()                       # the engine holds products' weights in its dtype ...
    f = lambda n: p[n].detach().float().double()                         # ... and biases / LayerNorm affines in fp32
    h0 = _rows(e.read("in").cpu().double(), 1, C_)[0]
    kv = e.read("kv").cpu().double()[0, :, :, 0].T                        # [keys, width]
    K, V = kv[:, info["ok"]:info["ok"] + C_], kv[:, info["ov"]:info["ov"] + C_]
    d = C_ // heads
    Wq, Wo, bo = w(TB + ".attn2.to_q.weight"), w(TB + ".attn2.to_out.0.weight"), f(TB + ".attn2.to_out.0.bias")
    g, b = f(TB + ".norm2.weight"), f(TB + ".norm2.bias")

    def fn(h):
        q = torch.nn.functional.layer_norm(h, (C_,), g, b, 1e-5) @ Wq.T
        o = torch.cat([_attend(q[:, i * d:(i + 1) * d], K[:, i * d:(i + 1) * d], V[:, i * d:(i + 1) * d], 1.0 / d ** 0.5, False) for i in range(heads)], -1)
        return o @ Wo.T + bo + h
    return fn, h0


def _reference(fn, h0, Vt, Ut):
    dO = torch.stack([torch.func.jvp(fn, (h0,), (v,))[1] for v in Vt.double()])
    hr = h0.clone().requires_grad_(True)
    y = fn(hr)
    gX = torch.stack([torch.autograd.grad(y, hr, u, retain_graph=True)[0] for u in Ut.double()])
    return dO, gX


def _tangents(C_, k, dtype, seed=0):
    g = torch.Generator().manual_seed(7 * C_ + k + seed)
    rnd = lambda t: t.to(dtype).float()
    return rnd(torch.randn(k, ROWS, C_, generator=g)), rnd(torch.randn(k, ROWS, C_, generator=g))


def _passes(e, Vt, Ut, C_):
    k = Vt.shape[0]
    dO = _rows(e.jvp_between("in", "out", _flat(Vt)).cpu(), k, C_)
    gX = _rows(e.vjp_between("in", "out", _flat(Ut)).cpu(), k, C_)
    return dO, gX


def _fold_info(e, index=0):
    _, l = _lib()
    v = (C.c_int64 * 12)()
    assert l.dpb_debug_cross_fold(e.h, index, v) == 0, l.dpb_last_error()
    return dict(zip(("op", "live", "C", "H", "rows", "keys", "Gt", "Gk", "F", "Fk", "P", "S1"), list(v)))


def _ws(e):
    return e._ws[(-e._ws.data_ptr()) % 256:]


# ------------------------------------------------------------------------------------------------ 1. route against route on one stash
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("C_,switch", CASES)
def test_folded_route_against_one_launch_route_and_fp64(C_, switch, dtype):
    """k = 1, 3, 5: 64, 192, 320 rows -- below one tile, a ragged last tile, several tiles of the 128 x 128 form of the epilogue (forced: at these
    row counts the dispatch picks the 64 x 128 form, which the same rows fill exactly) and one, three, five tiles of the 64 x 128 form.  One primal
    (switch on: the stash serves both routes)."""
    _set(switch)
    net, info = _run_primal(C_, dtype)
    e = net.engine
    assert _fold_info(e)["live"] == 1
    fn, h0 = _chain(C_, dtype, e, info)
    L, l = _lib()
    for k, tile in ((1, 0), (3, 0), (5, 0), (1, 515), (3, 515), (5, 515)):
        Vt, Ut = _tangents(C_, k, dtype)
        rdO, rgX = _reference(fn, h0, Vt, Ut)
        try:
            L.check(l.dpb_debug_set(b"gemm_tile", tile))
            _set(0)
            odO, ogX = _passes(e, Vt, Ut, C_)
            _set(switch)
            fdO, fgX = _passes(e, Vt, Ut, C_)
        finally:
            L.check(l.dpb_debug_set(b"gemm_tile", 0))
        for what, old, new, ref in (("jvp", odO, fdO, rdO), ("vjp", ogX, fgX, rgX)):
            # the chain's own part of the result: without the residual's identity both errors would be measured against a norm it dominates
            inp = (Vt if what == "jvp" else Ut).double()
            eo, en = rel(old.double() - inp, ref - inp), rel(new.double() - inp, ref - inp)
            print(f"C={C_} {dtype} k={k} tile={tile} {what}: one-launch route {eo:.3e}, folded route {en:.3e}")
            assert torch.isfinite(new).all()
            assert not torch.equal(old, new), "the switch did not change the route"
            assert en <= 1.5 * eo, (C_, dtype, k, tile, what, eo, en)


# ------------------------------------------------------------------------------------------------ 2. adjointness
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("C_,switch", CASES)
def test_folded_tangent_and_adjoint_are_adjoint(C_, switch, dtype):
    """<J v_i, u_j> against <v_i, J^T u_j> for 5 x 5 pairs: the folded route's disagreement is at most 1.5 x the one-launch route's (a swapped
    Gt / F or Gk / Fk orientation gives a disagreement of order one)."""
    _set(switch)
    net, _ = _run_primal(C_, dtype)
    e = net.engine
    Vt, Ut = _tangents(C_, 5, dtype, seed=1)
    gap = {}
    for name, v in (("old", 0), ("fold", switch)):
        _set(v)
        dO, gX = _passes(e, Vt, Ut, C_)
        # the chain without its residual, whose identity both sides share exactly
        a = torch.einsum("irc,jrc->ij", dO.double() - Vt.double(), Ut.double())
        b = torch.einsum("irc,jrc->ij", Vt.double(), gX.double() - Ut.double())
        gap[name] = float((a - b).norm() / a.norm())
    print(f"C={C_} {dtype} adjointness gap: one-launch route {gap['old']:.3e}, folded route {gap['fold']:.3e}")
    assert gap["fold"] <= 1.5 * gap["old"], gap


# ------------------------------------------------------------------------------------------------ 3. padding
@pytest.mark.parametrize("C_,switch", [(640, 1), (320, 2)])
def test_pad_rows_and_columns(C_, switch):
    """The 77 context rows are all there are.  Rows 77..127 of every head window of Gt / F are never written and never looked at: poisoned with
    NaN after the primal, tangent and adjoint results keep their bits.  Columns 77..79 of every head of the scratch are exact zeros."""
    dtype = torch.bfloat16
    _set(switch)
    net, _ = _run_primal(C_, dtype)
    e = net.engine
    fi = _fold_info(e)
    H, ws = fi["H"], _ws(e)
    view = lambda off, shape: ws[off:off + 2 * shape[0] * shape[1] * shape[2]].view(dtype).view(*shape)
    Gt, F = view(fi["Gt"], (H, 128, C_)), view(fi["F"], (H, 128, C_))
    assert (Gt[:, KEYS:] == 0).all() and (F[:, KEYS:] == 0).all() and Gt[:, :KEYS].abs().sum() > 0 and F[:, :KEYS].abs().sum() > 0
    Vt, Ut = _tangents(C_, 3, dtype, seed=2)
    clean = _passes(e, Vt, Ut, C_)
    try:
        Gt[:, KEYS:] = float("nan"); F[:, KEYS:] = float("nan")
        dO = _rows(e.jvp_between("in", "out", _flat(Vt)).cpu(), 3, C_)
        S = view(fi["S1"], (3 * ROWS, H, 80)).clone()
        gX = _rows(e.vjp_between("in", "out", _flat(Ut)).cpu(), 3, C_)
        S2 = view(fi["S1"], (3 * ROWS, H, 80)).clone()
    finally:
        Gt[:, KEYS:] = 0; F[:, KEYS:] = 0
    assert torch.equal(dO, clean[0]) and torch.equal(gX, clean[1])
    for s in (S, S2):
        assert torch.isfinite(s.float()).all() and (s[:, :, KEYS:] == 0).all() and s[:, :, :KEYS].abs().sum() > 0


# ------------------------------------------------------------------------------------------------ 4. launches
@pytest.mark.parametrize("C_,switch", [(640, 1), (1280, 1), (320, 2)])
def test_launch_counts(C_, switch):
    """one folded layer: tangent and adjoint passes enqueue one launch fewer each, the stashing primal four more; dpb_forward is unchanged.
    Every product unsplit (gemm_splitk = 1): at 64 rows the one-launch route's K = 1280 products split K and run a reduce kernel each, the
    folded route's K = 640 product does not -- the two reduce launches are the K-split plan's, not the route's."""
    dtype = torch.bfloat16
    net, _ = _net(C_, dtype)
    e = net.engine
    _, _, x, ctx = _params(C_, HEADS)
    L, l = _lib()
    n = {}
    try:
        L.check(l.dpb_debug_set(b"gemm_splitk", 1))
        _count_launches(e, n, switch, x, ctx, C_, dtype)
    finally:
        L.check(l.dpb_debug_set(b"gemm_splitk", 0))
    print(n)
    assert n["fold", "forward"] == n["old", "forward"]
    assert n["fold", "primal"] == n["old", "primal"] + 4
    for k in (1, 5):
        assert n["fold", "jvp", k] == n["old", "jvp", k] - 1 and n["fold", "vjp", k] == n["old", "vjp", k] - 1, (k, n)


def _count_launches(e, n, switch, x, ctx, C_, dtype):
    for name, v in (("old", 0), ("fold", switch)):
        _set(v)
        e.forward(x[:1], 500.0, ctx[:1], ("mid", 0))
        n[name, "forward"] = e.stats()[0]
        e.primal(x[:1], 500.0, ctx[:1], ("mid", 0))
        n[name, "primal"] = e.stats()[0]
        for k in (1, 5):
            Vt, Ut = _tangents(C_, k, dtype)
            e.jvp_between("in", "out", _flat(Vt))
            n[name, "jvp", k] = e.stats()[0]
            e.vjp_between("in", "out", _flat(Ut))
            n[name, "vjp", k] = e.stats()[0]


# ------------------------------------------------------------------------------------------------ 5. the rule
@pytest.mark.parametrize("what", ["C320", "sd21", "batch2"])
def test_rule_keeps_the_one_launch_route(what):
    """cross_fold = 1 leaves a C = 320 net, an SD-2.1-style net (head dim 64: 10 heads of C = 640) and a batch of two on the one-launch route:
    no operands are built and the whole-net tangent / adjoint passes are bit for bit those of cross_fold = 0"""
    dtype = torch.bfloat16
    C_, heads, batch = {"C320": (320, 8, 1), "sd21": (640, 10, 1), "batch2": (640, 8, 2)}[what]
    res = {}
    for v in (0, 1):
        _set(v)
        net, _ = _run_primal(C_, dtype, heads, batch, max_batch=batch)
        e = net.engine
        assert _fold_info(e)["live"] == 0
        g = torch.Generator().manual_seed(5)
        V = torch.randn(2 * batch, 4 * ROWS, generator=g)
        U = torch.randn(2 * batch, C_ * ROWS, generator=g)
        res[v] = (e.jvp(("mid", 0), V).cpu(), e.vjp(("mid", 0), U).cpu(), e.stats()[0])
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and res[0][2] == res[1][2]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_folded_route_is_bitwise_reproducible(dtype):
    """two runs of primal + whole-net tangent + adjoint on the folded route (C = 640, the rule) give identical bits"""
    _set(1)
    g = torch.Generator().manual_seed(6)
    V, U = torch.randn(5, 4 * ROWS, generator=g), torch.randn(5, 640 * ROWS, generator=g)
    runs = []
    for _ in range(2):
        net, _ = _run_primal(640, dtype)
        e = net.engine
        assert _fold_info(e)["live"] == 1
        runs.append((e.jvp(("mid", 0), V).cpu(), e.vjp(("mid", 0), U).cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
