"""The two tape additions of the guided-diffusion (ADM) kind at op level, through one-op tapes on a fresh engine (helpers of tests/_norm_ref.py):
the modulated (scale-shift) GroupNorm against an fp64 autograd reference, and the 2x2 resampling op against its own definition.

Modulated GroupNorm.  y = GN(x; gamma, beta) (1 + s_b) + h_b (+ SiLU), (s_b | h_b) a column window of a SHARED projection of the timestep
embedding.  Batch 3 at three distinct timesteps (three different embedding rows; a wrong row shows in the primal, a wrong j / kps mapping in the
tangents and cotangents, kps = 2) and at one shared timestep (row 0 for every sample).  Per-row errors (one row = one (tangent, group)), every row
compared.  Bounds: those of the plain op's kernel family (_norm_ref.BOUNDS: the formulas are the plain op's with gamma_b = gamma (1 + s_b),
beta_b = beta (1 + s_b) + h_b) plus 4 x 2^-24: gamma_b and beta_b carry up to two fp32 roundings each that a shared affine does not.  The
reference holds the embedding projection as the engine does: the fp64 product of the dtype-rounded operands, rounded to the engine dtype.
Routes: C = 40 / G = 4 takes the one-launch kernel at 2x2 and 6x10 and the two-pass kernels at 24x24; C = 8 / G = 2 and C = 136 / G = 17 take the
two-pass kernels at every size (their group windows are narrower than 64 bytes), C = 8 in 16-bit with fewer channels per group than a chunk.

Resampling.  Average pool and nearest upsample, primal, tangent and adjoint, the adjoint as first write and as accumulation (two resampling ops
reading one buffer).  The reference does the kernel's arithmetic in fp32 in the stated order (window sum in (dy, dx) order, times the scale,
plus the old value) and rounds once to the engine dtype; results must be within 1 ulp of it in the engine dtype (the accumulating 16-bit case
rounds twice, as the engine's stored cotangent does: first write, then sum).

An unmodulated GroupNorm (in1 = -1) must be bitwise the parent commit's: that is what the untouched bitwise and launch-count tests of the suite
(tests/test_gpu_norm_ops.py, test_gpu_launch_counts.py, test_gpu_timesteps.py) hold; no parent build is at hand inside the suite.
"""
import math

import pytest
import torch

import _norm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DT = [pytest.param(F32, id="fp32"), pytest.param(BF, id="bf16"), pytest.param(F16, id="fp16")]
EXTRA = 4 * 2.0 ** -24                                   # see the module docstring
TEMB = 8                                                 # width of the sinusoid feeding the projection
COL = 16                                                 # first column of the (scale | shift) window: not 0, so a dropped offset shows

GN_CASES = [(8, 2, (2, 2)), (8, 2, (6, 10)), (40, 4, (2, 2)), (40, 4, (6, 10)), (40, 4, (24, 24)), (136, 17, (2, 2)), (136, 17, (6, 10))]


def test_gn_cases_reach_both_kernels():
    routes = {(c, hw, dt): bool(R.gn_fused_groups(c, g, hw[0] * hw[1], dt)) for c, g, hw in GN_CASES for dt in (F32, BF)}
    assert any(routes.values()) and not all(routes.values())
    assert routes[(40, (6, 10), F32)] and not routes[(40, (24, 24), F32)] and not routes[(136, (6, 10), BF)]


def _sinusoid(t):
    """the engine's embedding for Engine(tape, TEMB, flip_sin_to_cos=False, half_minus_one=True): [sin | cos], exponent denominator half - 1"""
    half = TEMB // 2
    fr = torch.exp(torch.arange(half, dtype=torch.float32) * (-(math.log(10000.0) / (half - 1))))
    a = torch.tensor(t, dtype=torch.float32)[:, None] * fr[None]
    return torch.cat([torch.sin(a), torch.cos(a)], dim=1)


def _mod_tape(p, dtype, rows, C, G, silu):
    from diffusion_pullback_amd import lib as L
    from diffusion_pullback_amd.tape import Tape
    t = Tape(p, dtype, DEV)
    t.temb_in = t.buf(1, TEMB, L.BUF_SHARED)
    emb = t.conv("emb", t.temb_in, (1, 1), COL + 2 * C, ks=1, need_adj=False, kind=L.BUF_SHARED)
    t.x = t.buf(rows, C)
    o = t.groupnorm_mod("n", t.x, G, 1e-5, silu, emb, COL)
    t.tap("o", o, C, rows, 1)
    return t


@pytest.mark.parametrize("distinct", [True, False], ids=["t3", "t1"])
@pytest.mark.parametrize("silu", [False, True], ids=["plain", "silu"])
@pytest.mark.parametrize("C,G,hw", GN_CASES, ids=[f"C{c}-{h}x{w}" for c, _, (h, w) in GN_CASES])
@pytest.mark.parametrize("dtype", DT)
def test_modulated_groupnorm(dtype, C, G, hw, silu, distinct):
    from diffusion_pullback_amd.engine import Engine
    rows, B, kps = hw[0] * hw[1], 3, 2
    g = torch.Generator().manual_seed(1000 * C + rows + 7 * int(silu))
    p = R.norm_params(g, ["n"], C)
    p["emb.weight"] = 0.5 * torch.randn(COL + 2 * C, TEMB, generator=g)
    p["emb.bias"] = 0.1 * torch.randn(COL + 2 * C, generator=g)
    ts = [10.0, 200.0, 700.0] if distinct else [200.0] * 3
    x = R.plain_input(g, (B, rows, C), dtype)
    V = R.plain_input(g, (B * kps, rows, C), dtype)
    U = R.plain_input(g, (B * kps, rows, C), dtype)
    e = Engine(_mod_tape(p, dtype, rows, C, G, silu), TEMB, False, True, C, max_batch=B, max_tangents=B * kps)
    e.primal(R.to_nchw(x), ts, None, "o")
    O = e.read("o")[..., 0].permute(0, 2, 1)
    dO = R.from_flat(e.jvp("o", R.to_nchw(V).reshape(B * kps, -1)), rows)
    gX = R.from_flat(e.vjp("o", R.to_nchw(U).reshape(B * kps, -1)), rows)
    # fp64 reference; the projection as the engine holds it
    emb = R.rnd(R.rnd(_sinusoid(ts), dtype).double() @ R.rnd(p["emb.weight"], dtype).double().T + p["emb.bias"].double(), dtype).double()
    s, h = emb[:, COL:COL + C], emb[:, COL + C:COL + 2 * C]
    gam, bet = p["n.weight"].double(), p["n.bias"].double()

    def f(xx, idx):
        y = R.group_norm_ref(xx, gam, bet, G, 1e-5) * (1 + s[idx][:, None, :]) + h[idx][:, None, :]
        return y * torch.sigmoid(y) if silu else y
    xd = x.double()
    ib, it = torch.arange(B), torch.arange(B * kps) // kps
    with torch.no_grad():
        Or = f(xd, ib)
    _, dOr = torch.func.jvp(lambda a: f(a, it), (xd[it],), (V.double(),))
    xs = xd[it].clone().requires_grad_(True)
    (gXr,) = torch.autograd.grad(f(xs, it), xs, U.double())
    fam = "gn_fused" if R.gn_fused_groups(C, G, rows, dtype) else "gn_two_pass"
    for which, out, ref in (("primal", O, Or), ("tangent", dO, dOr), ("adjoint", gX, gXr)):
        rb, gb = R.bound(fam, dtype, which)
        worst = R.compare(out.cpu(), ref, G, rb + EXTRA, gb + EXTRA, f"{fam} {which} C={C} hw={hw} silu={silu} distinct={distinct}")
        print(fam, which, "worst row error", worst)
    if distinct:                                         # the rows really differ in their modulation
        assert (s[0] - s[1]).abs().max() > 1e-2 and (s[1] - s[2]).abs().max() > 1e-2


# ----------------------------------------------------------------------------------------------- resampling
def _pool(a, H, W, scale):
    """a [n, 2H*2W, C] fp32 -> [n, H*W, C]: window sum in (dy, dx) order, times scale (the kernel's order, fp32)"""
    n, _, C = a.shape
    a = a.reshape(n, H, 2, W, 2, C)
    acc = torch.zeros(n, H, W, C, dtype=torch.float32)
    for dy in range(2):
        for dx in range(2):
            acc = acc + a[:, :, dy, :, dx]
    return (acc * scale).reshape(n, H * W, C)


def _up(a, H, W, scale):
    """a [n, H*W, C] -> [n, 2H*2W, C]: scale * a[y // 2][x // 2]"""
    n, _, C = a.shape
    a = (a * scale).reshape(n, H, 1, W, 1, C).expand(n, H, 2, W, 2, C)
    return a.reshape(n, 4 * H * W, C)


def _ulps(out, ref, dtype):
    """distance in units of the engine dtype's last place (both rounded to it: the engine's outputs already are)"""
    it = torch.int32 if dtype == F32 else torch.int16
    a, b = out.to(dtype).contiguous().view(it).to(torch.int64), ref.to(dtype).contiguous().view(it).to(torch.int64)
    lo = -(1 << (31 if dtype == F32 else 15))
    a, b = torch.where(a < 0, lo - a, a), torch.where(b < 0, lo - b, b)      # sign-magnitude -> a monotone integer line (-0 and +0 coincide)
    return (a - b).abs().max().item()


def _resample_tape(dtype, H, W, C, up, twice):
    from diffusion_pullback_amd import lib as L
    from diffusion_pullback_amd.tape import Tape
    t = Tape({}, dtype, DEV)
    t.temb_in = t.buf(1, 8, L.BUF_SHARED)
    t.x = t.buf(H * W, C)
    o = t.resample(t.x, (H, W), up)
    if twice:                                            # two consumers of x: the adjoint of the op run second accumulates
        o = t.concat(o, t.resample(t.x, (H, W), up))
    t.tap("o", o, t.buffers[o][1], t.buffers[o][0], 1)
    return t


RS_CASES = [(False, 4, 4), (False, 12, 20), (True, 6, 10), (True, 2, 2)]     # (up, input H, input W): 4x4 -> 2x2, 12x20 -> 6x10, 6x10 -> 12x20


@pytest.mark.parametrize("twice", [False, True], ids=["first-write", "accumulate"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("C", [8, 40])
@pytest.mark.parametrize("up,H,W", RS_CASES, ids=[f"{'up' if u else 'pool'}-{h}x{w}" for u, h, w in RS_CASES])
@pytest.mark.parametrize("dtype", DT)
def test_resample(dtype, up, H, W, C, n, twice):
    e = R.engine(_resample_tape(dtype, H, W, C, up, twice), n, n)
    g = torch.Generator().manual_seed(H * 100 + W + C + n)
    rin = H * W
    rout = 4 * rin if up else rin // 4
    h, w = (H, W) if up else (H // 2, W // 2)                                # the small side
    x = R.plain_input(g, (n, rin, C), dtype)
    V = R.plain_input(g, (n, rin, C), dtype)
    U = R.plain_input(g, (n, rout, C * (2 if twice else 1)), dtype)
    fwd = (lambda a: _up(a, h, w, 1.0)) if up else (lambda a: _pool(a, h, w, 0.25))
    adj = (lambda a: _pool(a, h, w, 1.0)) if up else (lambda a: _up(a, h, w, 0.25))
    e.primal(R.to_nchw(x), 1.0, None, "o")               # (not R.run_engine: it takes the output to have the input's rows)
    O = e.read("o")[..., 0].permute(0, 2, 1)
    dO = R.from_flat(e.jvp("o", R.to_nchw(V).reshape(n, -1)), rout)
    gX = R.from_flat(e.vjp("o", R.to_nchw(U).reshape(n, -1)), rin)
    rep = (lambda a: torch.cat([a, a], dim=-1)) if twice else (lambda a: a)
    assert _ulps(O.cpu(), rep(R.rnd(fwd(x), dtype)), dtype) <= 1
    assert _ulps(dO.cpu(), rep(R.rnd(fwd(V), dtype)), dtype) <= 1
    if twice:                                            # reverse tape order: the second op writes first, the first accumulates onto the stored value
        ref = R.rnd(R.rnd(adj(U[..., C:]), dtype) + adj(U[..., :C]), dtype)
    else:
        ref = R.rnd(adj(U), dtype)
    d = _ulps(gX.cpu(), ref, dtype)
    print("resample", "up" if up else "pool", (H, W), C, n, "adjoint ulps", d)
    assert d <= 1


def test_resample_refuses_bad_shapes():
    from diffusion_pullback_amd import lib as L
    from diffusion_pullback_amd.tape import Tape
    t = Tape({}, F32, DEV)
    t.temb_in = t.buf(1, 8, L.BUF_SHARED)
    t.x = t.buf(15, 8)
    o = t.buf(3, 8)
    t._op(kind=L.OP_RESAMPLE, in0=t.x, out=o, ip=[0, 3, 5] + [0] * 9)       # odd sides cannot be pooled 2x2
    t.tap("o", o, 8, 3, 1)
    with pytest.raises(L.DpbError, match="resample"):
        R.engine(t, 1, 1)
