"""Op-level checks of the normalisation and pointwise kernels (csrc/norm.hip, csrc/elementwise.hip): tiny tapes, an fp64 reference of the same
composition, input generators and a per-row comparator.  Modelled on tests/_attn_ref.py.

A net is a list of steps (dicts made by gn / ln / geglu / unary / concat / linear below); `build_tape` turns it into an engine tape and
`evaluate` restates it in plain fp64 torch, so the two always describe the same composition.  Layout convention: activations are
[batch, rows, channels] (the engine's NHWC rows; its NCHW interface sees [batch, channels, rows, 1]); tangents / cotangents are [nt, rows, channels]
with tangent j belonging to sample j // kps, as in the engine.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
UNIT = {F32: 2.0 ** -24, BF: 2.0 ** -8, F16: 2.0 ** -11}          # unit roundoff of the engine dtypes
LADDER = ((0.0, 1.0), (8.0, 1.0), (64.0, 0.25), (256.0, 0.25))    # (|group or row mean|, spread) rungs of the offset ladder


def ladder_rungs(dtype):
    """bf16 resolves 0.5 at 64 (the 0.25 spread would be rounding noise): first two rungs; fp16 (0.0625 at 64, 0.25 at 256): first three"""
    return LADDER[:{BF: 2, F16: 3, F32: 4}[dtype]]


def rnd(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """the values the engine sees: fp32 input rounded to the engine dtype, back in fp32"""
    return t.float().to(dtype).float()


# =============================================================================================== nets
def gn(out, src, name, G=32, eps=1e-5, silu=False):
    return dict(op="gn", out=out, src=src, name=name, G=G, eps=eps, silu=silu)


def ln(out, src, name, eps=1e-5):
    return dict(op="ln", out=out, src=src, name=name, eps=eps)


def geglu(out, src, il=0):
    return dict(op="geglu", out=out, src=src, il=il)


def unary(out, src, fn):
    """fn: silu | quick_gelu | gelu (primal-only ops of the engine)"""
    return dict(op=fn, out=out, src=src)


def concat(out, a, b):
    return dict(op="concat", out=out, src=a, src2=b)


def linear(out, src, name, cout, res=None, interleave=0):
    """ks = 1 product y = x W^T + b (+ res); interleave = 64: the output columns in the a0 g0 a1 g1 ... layout of a GEGLU projection (Tape.conv)"""
    return dict(op="linear", out=out, src=src, name=name, cout=cout, res=res, interleave=interleave)


def build_tape(steps: List[dict], params: Dict[str, torch.Tensor], dtype, device, rows: int, ch: int):
    """the engine tape of a net on x [rows][ch]; the last step's output is the tap "o" """
    from diffusion_pullback_amd import lib as L
    from diffusion_pullback_amd.tape import Tape
    t = Tape(params, dtype, device)
    t.temb_in = t.buf(1, 8, L.BUF_SHARED)
    t.x = t.buf(rows, ch)
    b = {"x": t.x}
    for s in steps:
        op, src = s["op"], b[s["src"]]
        if op == "gn":
            o = t.groupnorm(s["name"], src, s["G"], s["eps"], s["silu"])
        elif op == "ln":
            o = t.layernorm(s["name"], src, s["eps"])
        elif op == "geglu":
            o = t.geglu(src, s["il"])
        elif op in ("silu", "quick_gelu", "gelu"):
            o = getattr(t, op)(src)
        elif op == "concat":
            o = t.concat(src, b[s["src2"]])
        elif op == "linear":
            o = t.conv(s["name"], src, (rows, 1), s["cout"], ks=1, res=b[s["res"]] if s["res"] else -1, interleave=s.get("interleave", 0))
        else:
            raise ValueError(op)
        b[s["out"]] = o
    last = b[steps[-1]["out"]]
    t.tap("o", last, t.buffers[last][1], rows, 1)
    return t


def engine(tape, batch: int, tangents: int):
    from diffusion_pullback_amd.engine import Engine
    return Engine(tape, 8, False, True, tape.buffers[tape.x][1], max_batch=batch, max_tangents=tangents)


def to_nchw(x: torch.Tensor) -> torch.Tensor:
    """[B, rows, C] -> [B, C, rows, 1]"""
    return x.permute(0, 2, 1).unsqueeze(-1).contiguous()


def from_flat(y: torch.Tensor, rows: int) -> torch.Tensor:
    """engine result [n, C * rows] (NCHW-flattened) -> [n, rows, C]"""
    return y.reshape(y.shape[0], -1, rows).permute(0, 2, 1)


# =============================================================================================== fp64 restatement
def interleave_perm(F: int, il: int) -> torch.Tensor:
    """column i of a 64-interleaved [..][2F] GEGLU input is column perm[i] of the split (a | g) layout: a-block 0, g-block 0, a-block 1, ...
    (the row permutation Tape._conv_w applies to the FF-in weight)"""
    blk = torch.arange(F).reshape(F // il, il)
    return torch.stack([blk, blk + F], dim=1).reshape(-1)


def gelu_erf(g: torch.Tensor) -> torch.Tensor:
    return 0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0)))


def group_norm_ref(a, gamma, beta, G, eps, silu=False):
    """a [n, rows, C]: mean and biased variance per (sample, group) over rows x C/G, eps, affine, optional SiLU"""
    n, R, C = a.shape
    g = a.reshape(n, R, G, C // G)
    mean = g.mean(dim=(1, 3), keepdim=True)
    var = (g - mean).pow(2).mean(dim=(1, 3), keepdim=True)
    y = ((g - mean) / torch.sqrt(var + eps)).reshape(n, R, C) * gamma + beta
    return y * torch.sigmoid(y) if silu else y


def layer_norm_ref(a, gamma, beta, eps):
    mean = a.mean(-1, keepdim=True)
    var = (a - mean).pow(2).mean(-1, keepdim=True)
    return (a - mean) / torch.sqrt(var + eps) * gamma + beta


def geglu_ref(a, il=0):
    F = a.shape[-1] // 2
    if il:
        a = a[..., torch.argsort(interleave_perm(F, il)).to(a.device)]        # back to the split layout
    return a[..., :F] * gelu_erf(a[..., F:])


def evaluate(steps: List[dict], params: Dict[str, torch.Tensor], x: torch.Tensor, dtype) -> torch.Tensor:
    """the net in fp64 on x [n, rows, C]; weights of products are the values the engine holds (rounded to its dtype), norm affines and biases fp32"""
    v = {"x": x}
    P = lambda n: params[n].to(device=x.device, dtype=torch.float64)
    for s in steps:
        op, a = s["op"], v[s["src"]]
        if op == "gn":
            y = group_norm_ref(a, P(s["name"] + ".weight"), P(s["name"] + ".bias"), s["G"], s["eps"], s["silu"])
        elif op == "ln":
            y = layer_norm_ref(a, P(s["name"] + ".weight"), P(s["name"] + ".bias"), s["eps"])
        elif op == "geglu":
            y = geglu_ref(a, s["il"])
        elif op == "silu":
            y = a * torch.sigmoid(a)
        elif op == "quick_gelu":
            y = a * torch.sigmoid(1.702 * a)
        elif op == "gelu":
            y = gelu_erf(a)
        elif op == "concat":
            y = torch.cat([a, v[s["src2"]]], dim=-1)
        elif op == "linear":
            W = rnd(params[s["name"] + ".weight"], dtype).to(device=x.device, dtype=torch.float64)
            y = a @ W.T
            if s["name"] + ".bias" in params:
                y = y + P(s["name"] + ".bias")
            if s["res"]:
                y = y + v[s["res"]]
            if s.get("interleave"):
                y = y[..., interleave_perm(s["cout"] // 2, s["interleave"]).to(y.device)]
        else:
            raise ValueError(op)
        v[s["out"]] = y
    return v[steps[-1]["out"]]


def reference(steps, params, x: torch.Tensor, dtype, V: Optional[torch.Tensor] = None, U: Optional[torch.Tensor] = None, kps: int = 1):
    """fp64 primal / tangent / adjoint of the net by autograd.  x [B, rows, C] (already rounded to the engine dtype); V [nt, rows, C], U [nt, rows,
    Cout]: tangent / cotangent j belongs to sample j // kps.  Returns (O, dO, gX) in fp64 (None where not asked)."""
    x = x.double()
    f = lambda xx: evaluate(steps, params, xx, dtype)
    with torch.no_grad():
        O = f(x)
    dO = gX = None
    if V is not None:
        idx = torch.arange(V.shape[0], device=x.device) // kps
        _, dO = torch.func.jvp(f, (x[idx],), (V.double(),))
    if U is not None:
        idx = torch.arange(U.shape[0], device=x.device) // kps
        xs = x[idx].clone().requires_grad_(True)
        (gX,) = torch.autograd.grad(f(xs), xs, U.double())
    return O, dO, gX


def run_engine(e, x: torch.Tensor, V: Optional[torch.Tensor], U: Optional[torch.Tensor], forward_only: bool = False):
    """x [B, rows, C], V [nt, rows, C], U [nt, rows, Cout] (device fp32) -> (O, dO, gX) as [., rows, ch] fp32 and the launch counts of the passes"""
    rows = x.shape[1]
    n = {}
    if forward_only:
        O = e.forward(to_nchw(x), 1.0, None, "o")[..., 0].permute(0, 2, 1)
        return O, None, None, {"primal": e.stats()[0]}
    e.primal(to_nchw(x), 1.0, None, "o")
    n["primal"] = e.stats()[0]
    O = e.read("o")[..., 0].permute(0, 2, 1)
    dO = gX = None
    if V is not None:
        dO = from_flat(e.jvp("o", to_nchw(V).reshape(V.shape[0], -1)), rows)
        n["tangent"] = e.stats()[0]
    if U is not None:
        gX = from_flat(e.vjp("o", to_nchw(U).reshape(U.shape[0], -1)), rows)
        n["adjoint"] = e.stats()[0]
    return O, dO, gX, n


# =============================================================================================== inputs
def affine(g: torch.Generator, C: int):
    """gamma ~ 1 + 0.5 randn, beta ~ 0.5 randn: the all-ones default would hide a swapped or mis-indexed affine"""
    return 1.0 + 0.5 * torch.randn(C, generator=g), 0.5 * torch.randn(C, generator=g)


def norm_params(g: torch.Generator, names, C: int) -> Dict[str, torch.Tensor]:
    p = {}
    for n in names:
        p[n + ".weight"], p[n + ".bias"] = affine(g, C)
    return p


def plain_input(g: torch.Generator, shape, dtype, scale: float = 1.0) -> torch.Tensor:
    return rnd(scale * torch.randn(*shape, generator=g), dtype)


def ladder_input(g: torch.Generator, B: int, rows: int, C: int, dtype, m: float, s: float, groups: int = 0) -> torch.Tensor:
    """every group (groups > 0: per (sample, group), constant over rows and the group's channels) or every token row (groups = 0) gets its own mean,
    drawn from +-m, plus s * randn"""
    if groups:
        sign = torch.randint(0, 2, (B, 1, groups, 1), generator=g).float() * 2 - 1
        off = (sign * m).expand(B, rows, groups, C // groups).reshape(B, rows, C)
    else:
        off = (torch.randint(0, 2, (B, rows, 1), generator=g).float() * 2 - 1) * m
    return rnd(off + s * torch.randn(B, rows, C, generator=g), dtype)


# =============================================================================================== comparator
def row_errors(out: torch.Tensor, ref: torch.Tensor, groups: int = 0, tau: float = 0.05) -> torch.Tensor:
    """out, ref [T, rows, C].  groups > 0 (GroupNorm): one "row" is one (tangent, group), all its rows x C/groups values -> [T, groups];
    groups = 0 (LayerNorm, GEGLU, ...): one token row -> [T, rows].  Error = |d row|_2 / (|ref row|_2 + tau * rms row norm of that tangent)."""
    T, R, C = ref.shape
    o, r = out.double(), ref.double()
    if groups:
        o = o.reshape(T, R, groups, C // groups).permute(0, 2, 1, 3).reshape(T, groups, -1)
        r = r.reshape(T, R, groups, C // groups).permute(0, 2, 1, 3).reshape(T, groups, -1)
    rn = r.norm(dim=-1)
    rms = rn.pow(2).mean(-1, keepdim=True).sqrt()
    return (o - r).norm(dim=-1) / (rn + tau * rms + 1e-300)


def errors(out: torch.Tensor, ref: torch.Tensor, groups: int = 0):
    """-> (largest row error, global relative error); every row of every output takes part"""
    out = out.to(ref.device)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    return float(row_errors(out, ref, groups).max()), float((out.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


def compare(out: torch.Tensor, ref: torch.Tensor, groups: int, row_bound: float, glob_bound: float, what: str = "", measured: Optional[dict] = None) -> float:
    """asserts finiteness, every row error <= row_bound and the global relative error <= glob_bound; returns the worst row error.  A failure
    names the worst (tangent, row).  `measured`: dict collecting (row, global) maxima per label."""
    out = out.to(ref.device)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    assert torch.isfinite(out).all(), f"{what}: non-finite output ({(~torch.isfinite(out)).sum().item()} elements)"
    e = row_errors(out, ref, groups)
    worst = float(e.max())
    t, r = [int(i) for i in torch.unravel_index(e.argmax(), e.shape)]
    glob = float((out.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))
    if measured is not None:
        m = measured.setdefault(what.split(" ")[0], [0.0, 0.0])
        m[0] = max(m[0], worst); m[1] = max(m[1], glob)
    assert worst <= row_bound, f"{what}: row error {worst:.3e} > {row_bound:.1e} at (tangent {t}, {'group' if groups else 'row'} {r}); global {glob:.3e}"
    assert glob <= glob_bound, f"{what}: global relative error {glob:.3e} > {glob_bound:.1e}"
    return worst


# (family, engine dtype) -> {pass: (row bound, global bound)}: twice the largest error measured on an MI355X over the cases of the family
# (tests/test_gpu_norm_ops.py; maxima in its docstring).  Inputs are zero-mean randn; the offset ladder has its own 8x-of-torch condition.
BOUNDS = {
    ("gn_fused", F32): {"primal": (5.0e-07, 1.9e-07), "tangent": (5.0e-07, 2.2e-07), "adjoint": (5.1e-07, 2.2e-07)},
    ("gn_fused", BF): {"primal": (4.0e-03, 3.4e-03), "tangent": (3.7e-03, 3.4e-03), "adjoint": (4.0e-03, 3.4e-03)},
    ("gn_fused", F16): {"primal": (4.7e-04, 4.3e-04), "tangent": (4.9e-04, 4.3e-04), "adjoint": (4.8e-04, 4.2e-04)},
    ("gn_two_pass", F32): {"primal": (8.2e-07, 2.0e-07), "tangent": (7.7e-07, 2.1e-07), "adjoint": (7.7e-07, 2.1e-07)},
    ("gn_two_pass", BF): {"primal": (4.3e-03, 3.5e-03), "tangent": (4.4e-03, 3.6e-03), "adjoint": (4.6e-03, 3.5e-03)},
    ("gn_two_pass", F16): {"primal": (5.3e-04, 4.3e-04), "tangent": (5.6e-04, 4.4e-04), "adjoint": (5.7e-04, 4.4e-04)},
    ("gn_atomic", F32): {"primal": (4.1e-07, 1.7e-07), "tangent": (4.0e-07, 2.0e-07), "adjoint": (3.4e-07, 1.9e-07)},
    ("gn_atomic", BF): {"primal": (3.9e-03, 3.4e-03), "tangent": (4.0e-03, 3.4e-03), "adjoint": (4.3e-03, 3.4e-03)},
    ("gn_atomic", F16): {"primal": (4.8e-04, 4.2e-04), "tangent": (5.0e-04, 4.2e-04), "adjoint": (4.8e-04, 4.3e-04)},
    ("ln", F32): {"primal": (2.9e-07, 1.4e-07), "tangent": (3.8e-07, 1.6e-07), "adjoint": (3.2e-07, 1.6e-07)},
    ("ln", BF): {"primal": (4.6e-03, 3.5e-03), "tangent": (4.7e-03, 3.5e-03), "adjoint": (4.9e-03, 3.6e-03)},
    ("ln", F16): {"primal": (5.4e-04, 4.2e-04), "tangent": (5.9e-04, 4.3e-04), "adjoint": (5.6e-04, 4.4e-04)},
    ("acc_gn", F32): {"primal": (2.7e-07, 1.6e-07), "tangent": (3.3e-07, 1.9e-07), "adjoint": (3.3e-07, 1.9e-07)},
    ("acc_gn", BF): {"primal": (3.8e-03, 3.4e-03), "tangent": (3.8e-03, 3.4e-03), "adjoint": (4.8e-03, 4.2e-03)},
    ("acc_gn", F16): {"primal": (4.6e-04, 4.3e-04), "tangent": (4.7e-04, 4.2e-04), "adjoint": (6.6e-04, 5.2e-04)},
    ("acc_ln", F32): {"primal": (2.9e-07, 1.2e-07), "tangent": (3.2e-07, 1.4e-07), "adjoint": (3.3e-07, 1.5e-07)},
    ("acc_ln", BF): {"primal": (3.7e-03, 3.4e-03), "tangent": (3.6e-03, 3.4e-03), "adjoint": (4.6e-03, 4.2e-03)},
    ("acc_ln", F16): {"primal": (4.4e-04, 4.2e-04), "tangent": (4.9e-04, 4.2e-04), "adjoint": (6.5e-04, 5.2e-04)},
    ("slab_gn", F32): {"primal": (1.2e-06, 9.3e-07), "tangent": (1.8e-06, 1.3e-06), "adjoint": (1.7e-06, 1.3e-06)},
    ("slab_gn", BF): {"primal": (6.9e-03, 5.6e-03), "tangent": (7.9e-03, 5.9e-03), "adjoint": (8.0e-03, 5.9e-03)},
    ("slab_gn", F16): {"primal": (8.9e-04, 7.1e-04), "tangent": (9.1e-04, 7.4e-04), "adjoint": (9.4e-04, 7.5e-04)},
    ("slab_ln", F32): {"primal": (7.5e-07, 6.9e-07), "tangent": (9.8e-07, 8.6e-07), "adjoint": (9.6e-07, 8.5e-07)},
    ("slab_ln", BF): {"primal": (5.9e-03, 5.4e-03), "tangent": (6.8e-03, 5.8e-03), "adjoint": (6.6e-03, 5.8e-03)},
    ("slab_ln", F16): {"primal": (7.2e-04, 6.7e-04), "tangent": (8.5e-04, 7.3e-04), "adjoint": (9.3e-04, 7.3e-04)},
    ("geglu", F32): {"primal": (1.4e-07, 7.2e-08), "tangent": (2.5e-07, 1.2e-07), "adjoint": (1.7e-07, 9.3e-08)},
    ("geglu", BF): {"primal": (4.9e-03, 3.4e-03), "tangent": (7.6e-03, 4.1e-03), "adjoint": (7.2e-03, 4.1e-03)},
    ("geglu", F16): {"primal": (6.5e-04, 4.5e-04), "tangent": (9.6e-04, 5.2e-04), "adjoint": (9.5e-04, 6.5e-04)},
    ("unary", F32): {"primal": (1.7e-07, 9.5e-08)},
    ("unary", BF): {"primal": (4.4e-03, 3.1e-03)},
    ("unary", F16): {"primal": (5.6e-04, 3.8e-04)},
    ("concat", F32): {"primal": (2.6e-07, 1.5e-07), "tangent": (4.4e-07, 2.0e-07), "adjoint": (4.2e-07, 2.1e-07)},
    ("concat", BF): {"primal": (8.9e-03, 4.1e-03), "tangent": (9.9e-03, 5.0e-03), "adjoint": (1.2e-02, 5.1e-03)},
    ("concat", F16): {"primal": (7.7e-04, 5.1e-04), "tangent": (1.6e-03, 6.3e-04), "adjoint": (1.7e-03, 6.4e-04)},
    # the fused product epilogues (tests/test_gpu_epilogue_ops.py; maxima in its docstring)
    ("epi_geglu", F32): {"primal": (8.4e-07, 6.0e-07), "tangent": (9.8e-07, 6.2e-07), "adjoint": (9.6e-07, 7.3e-07)},
    ("epi_geglu", BF): {"primal": (1.3e-02, 7.1e-03), "tangent": (1.5e-02, 7.2e-03), "adjoint": (1.4e-02, 7.2e-03)},
    ("epi_geglu", F16): {"primal": (1.4e-03, 8.8e-04), "tangent": (1.8e-03, 9.0e-04), "adjoint": (1.7e-03, 9.0e-04)},
    ("epi_geglu_fwd", F32): {"primal": (8.4e-07, 6.0e-07)},
    ("epi_geglu_fwd", BF): {"primal": (1.3e-02, 7.1e-03)},
    ("epi_geglu_fwd", F16): {"primal": (1.4e-03, 8.8e-04)},
    ("epi_ln", F32): {"primal": (1.0e-06, 7.1e-07), "tangent": (1.2e-06, 7.8e-07), "adjoint": (9.2e-07, 7.3e-07)},
    ("epi_ln", BF): {"primal": (8.0e-03, 6.1e-03), "tangent": (9.1e-03, 6.5e-03), "adjoint": (8.5e-03, 6.3e-03)},
    ("epi_ln", F16): {"primal": (1.1e-03, 7.4e-04), "tangent": (1.2e-03, 8.2e-04), "adjoint": (1.1e-03, 8.0e-04)},
}


def bound(family: str, dtype, which: str):
    return BOUNDS[(family, dtype)][which]


# =============================================================================================== the route rules of norm.hip, restated
def gn_fused_groups(C: int, G: int, HW: int, dtype) -> int:
    """gn_fused_groups: groups per window of the one-launch kernel, 0 = two passes"""
    CH, es = (4, 4) if dtype == F32 else (8, 2)
    cpg = C // G
    if cpg < CH:
        return 0
    gc = 1
    while gc <= G and gc <= 32:
        cw = gc * cpg
        if G % gc or cw % CH or cw * es < 64 or cw // CH > 16:
            gc *= 2
            continue
        ppi = 512 // (cw // CH)
        return gc if (HW + ppi - 1) // ppi <= 4 else 0
    return 0


def gn_route(C: int, G: int, HW: int, dtype, n: int, det: bool = True, primal: bool = True):
    """(route, launches) of gn_launch for n samples (primal) or tangents: "fused" 1; "red" 2 (the apply pass adds the block partials, at most
    GN_RED_MAX = 256 statistics blocks); "reduce" 3 (gn_reduce_kernel); "atomic" 3 primal (with gn_finalize) / 2"""
    if gn_fused_groups(C, G, HW, dtype):
        return "fused", 1
    if not det:
        return "atomic", 3 if primal else 2
    ppb = 64
    while ppb > 8 and ((HW + ppb - 1) // ppb) * n < 512:
        ppb >>= 1
    return ("red", 2) if (HW + ppb - 1) // ppb <= 256 else ("reduce", 3)


def ln_route(C: int, dtype) -> str:
    """ln_launch: "rows<LPR>x<NI>" (ln_rows_kernel) or "wave<MAXI>" (ln_kernel)"""
    nch = C // (4 if dtype == F32 else 8)
    for lpr in (8, 16, 32):
        if nch % lpr == 0 and nch // lpr in (3, 5):
            return f"rows{lpr}x{nch // lpr}"
    need = (nch + 63) // 64
    return f"wave{need if need <= 3 else 5}"
