"""Random small tapes against an fp64 restatement: the graph bookkeeping of csrc/engine.cpp (first-write / accumulate flags of the adjoint pass, the
residual hand-over, the parked split-K product, the ops a fused epilogue swallows, the activity flags of a pass seeded mid-graph, the concat adjoint
and the zeroed window of an inactive concat operand, the reset of all of it between passes) with every kernel already pinned at op level.
Modelled on tests/_product_ref.py and tests/_norm_ref.py, whose step dicts (`cv`, `gn`, `ln`, `geglu`, `concat`), `rnd`, `UNIT`, reference
functions and row-error comparator are reused; two step kinds are new here (`attn`, `resample`).

A tape is a `Graph`: an (H, W) image (plain rows: (rows, 1)) of `cin` channels, a step list, the named taps (a tap's name is its buffer's), and the
(src, dst) tap pairs of the `_between` passes.  `random_tape(seed, tier)` is deterministic in (seed, tier) and builds a DAG: buffers are read by
several ops, as input, as residual and as concat operand.  `build_tape` turns a Graph into an engine tape, `evaluate` restates it in fp64 torch on
NCHW tensors (the layout of the engine's boundary), `reference` takes the primal at every tap, J V by torch.func.jvp and J^T U by autograd from x
and from every inner src, and the forward seeded at src.  Tangent / cotangent j belongs to sample j // kps.

Rules of the engine the generator encodes (a tape that breaks one is refused at create time or is outside the reference's reach):
  * GEGLU_SOLE_INPUT: the input buffer of a GEGLU op has no other consumer and is no tap (the primal pass overwrites it in place).
  * PADDED_NOT_CONCATENATED: a buffer whose channel count is no multiple of 8 (cout = 4) is read by products and taps only, never by a concat
    (its padding channels would land in the middle of the wider buffer) and is no src of a between pass.
  * ATTENTION_ACTIVITY: q, k and v of an attention op depend on a between pass's src as they depend on x (seed_flags); motifs are atomic, a tap
    lies between motifs, never inside one.
  * SRC_IS_ACTIVATION: the src of a between pass is an op's output that depends on x; dst lies downstream of it.

Exact tier
----------
Linear ops only, weights sparse with entries in {-1, 0, 1}, x, V, U and the h of forward_from in {-1, 0, 1}, t = 0 (the sinusoid is 0 | 1).  The
only non-integer factor is the 0.25 of the 2x2 average pool (and of its adjoint); with P pool ops on the tape every value of every pass is a
multiple of 4^-P.  `magnitudes` evaluates the same net on absolute values for the primal, every tangent and every adjoint pass -- for the adjoint
the absolute cotangent of EVERY buffer, i.e. the sum of all its contributions, which bounds every partial sum the engine stores on the way.  If
magnitude x 4^P < 2^8 everywhere, every stored value and every partial sum in any order is (an integer below 2^8) x 4^-P: exact in bf16 (8
significant bits), fp16 and fp32, and exact in the fp32 accumulators, so rounding order cannot matter and the engine must return
ref64.float().to(dtype) bit for bit.  `random_tape` redraws weights and inputs (sparser with every attempt, same structure) until that holds
(`check_exact_precondition` asserts it), so one corpus serves the three dtypes.

Real tier
---------
Two to four motifs per tape (DDPM ResBlock with and without a 1x1 shortcut, GroupNorm + fused qkv + self-attention + projection with residual, the
SD transformer block at C = 320, cross-attention on a 77-row context) behind a 3x3 input convolution, composed with a long-skip concat, a stride-2
and an upsampling convolution, and a fan-out (a motif input that is a tap as well, or feeds two motifs).  Inputs are Gaussians rounded to the
engine dtype; sample 1 is an independent draw at twice the scale of sample 0, so a tangent linearised at the wrong sample is far off.
`reference(..., store=dtype)` rounds every stored buffer (primal, tangent and cotangent) to the dtype: the error of an ideal engine.

`drop(g, dtype, feature)` is the reference with one bookkeeping contribution removed (`feature_instances` lists them): one consumer's cotangent /
tangent, one residual, one inactive concat window that keeps another pass's tangent, sample j used instead of j // kps.
"""
from __future__ import annotations

import math
import random
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

from _norm_ref import BF, F16, F32, UNIT, rnd, gn, ln, geglu, concat, affine, group_norm_ref, layer_norm_ref, geglu_ref, interleave_perm, row_errors  # noqa: F401
from _product_ref import cv, names_of, r8, TEMB, RB_PAD, temb_rows, _conv, compare_exact  # noqa: F401

EXACT_SEEDS = tuple(range(40))
REAL_SEEDS = tuple(range(12))
EXACT_CH = (8, 16, 24, 40)
EXACT_SHAPES = ((4, 4), (8, 8), (6, 10), (7, 1), (77, 1))       # images; plain rows are (rows, 1).  HW = 60 is no multiple of 32
REAL_SHAPES = ((4, 4), (8, 8), (6, 10))
CTX = (77, 64)                                                  # rows and width of the cross-attention context


# =============================================================================================== steps
def attn(out, src, heads, c, kv=None):
    """self-attention over the q | k | v windows of src [rows][3c] (kv None), or cross-attention of q = src [rows][c] with the (k, v) projections
    kv = (k name, v name) of the constant context"""
    return dict(op="attn", out=out, src=src, heads=heads, c=c, kv=kv)


def resample(out, src, up):
    """2x2 average pool (up False) or nearest x2 upsample"""
    return dict(op="resample", out=out, src=src, up=up)


def kind(s) -> str:
    return s.get("op", "conv")


def inputs_of(s) -> List[Tuple[str, str]]:
    """(role, buffer) of every buffer the step reads: src; src2 of a concat; res of a product"""
    r = [("src", s["src"])]
    if kind(s) == "concat":
        r.append(("src2", s["src2"]))
    if kind(s) == "conv" and s["res"]:
        r.append(("res", s["res"]))
    return r


@dataclass
class Graph:
    seed: int
    tier: str
    hw: Tuple[int, int]
    cin: int
    steps: List[dict]
    taps: List[str]                                   # tape order; the last one is the end of the x-seeded passes
    pairs: List[Tuple[str, str]]
    B: int
    kps: int
    meta: Dict[str, Tuple[int, Tuple[int, int]]]      # buffer -> (channels, (H, W))
    motifs: List[str] = field(default_factory=list)
    ctx: Optional[Tuple[int, int]] = None
    t: float = 0.0
    attempt: int = 0
    params: Dict[str, torch.Tensor] = field(default_factory=dict)
    x: Optional[torch.Tensor] = None
    ctx_in: Optional[torch.Tensor] = None
    V: List[torch.Tensor] = field(default_factory=list)          # one per pass of `passes`
    U: List[torch.Tensor] = field(default_factory=list)
    Hsrc: Dict[str, torch.Tensor] = field(default_factory=dict)   # the activation forward_from plants at src

    def __iter__(self):
        return iter((self.steps, self.taps, self.pairs))

    @property
    def last(self) -> str:
        return self.taps[-1]

    @property
    def passes(self) -> List[Tuple[str, str]]:
        return [("x", self.last)] + list(self.pairs)

    @property
    def nt(self) -> int:
        return self.B * self.kps

    def producer(self, buf: str) -> int:
        return -1 if buf == "x" else next(i for i, s in enumerate(self.steps) if s["out"] == buf)

    def shape(self, buf: str, n: int) -> Tuple[int, int, int, int]:
        c, (h, w) = self.meta[buf]
        return (n, c, h, w)

    def active(self, src: str) -> Tuple[set, List[bool]]:
        """(buffers downstream of src, src included; per step: does it read one) -- seed_flags of engine.cpp"""
        b, on = {src}, []
        for i, s in enumerate(self.steps):
            a = i > self.producer(src) and any(n in b for _, n in inputs_of(s))
            on.append(a)
            if a:
                b.add(s["out"])
        return b, on

    def upstream(self, dst: str) -> set:
        """steps whose output reaches dst"""
        need, ops = {dst}, set()
        for i in range(self.producer(dst), -1, -1):
            if self.steps[i]["out"] in need:
                ops.add(i)
                need.update(n for _, n in inputs_of(self.steps[i]))
        return ops


class _Builder:
    def __init__(self, hw, cin):
        self.steps: List[dict] = []
        self.meta = {"x": (cin, tuple(hw))}
        self.n = 0

    def _new(self) -> str:
        self.n += 1
        return f"b{self.n}"

    def conv(self, src, cout, ks=1, stride=1, pad=1, up=False, res=None, rowbias=False, fused=None, interleave=0, bias=True, names=None):
        out = self._new()
        name = "w_" + out
        if fused:
            name = tuple((f"{name}_{i}", c, i != 1) for i, c in enumerate(fused))      # the middle projection has no bias
            cout = sum(fused)
        if names:
            name = names
        s = cv(out, src, name, cout, ks=ks, stride=stride, pad=pad, up=up, res=res, bias=bias, rowbias=rowbias)
        s["interleave"] = interleave
        h, w = self.meta[src][1]
        if ks == 1:
            ohw = (h, w)
        elif up:
            ohw = (2 * h, 2 * w)
        else:
            ohw = ((h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1) if pad else ((h + 1 - ks) // stride + 1, (w + 1 - ks) // stride + 1)
        self.steps.append(s)
        self.meta[out] = (cout, ohw)
        return out

    def add(self, s, c, hw) -> str:
        self.steps.append(s)
        self.meta[s["out"]] = (c, tuple(hw))
        return s["out"]

    def concat(self, a, b):
        assert self.meta[a][0] % 8 == 0 and self.meta[b][0] % 8 == 0, "PADDED_NOT_CONCATENATED"
        return self.add(concat(self._new(), a, b), self.meta[a][0] + self.meta[b][0], self.meta[a][1])

    def resample(self, a, up):
        h, w = self.meta[a][1]
        return self.add(resample(self._new(), a, up), self.meta[a][0], (2 * h, 2 * w) if up else (h // 2, w // 2))

    def gn(self, a, G, silu):
        o = self._new()
        return self.add(gn(o, a, "n_" + o, G=G, silu=silu), *self.meta[a])

    def ln(self, a):
        o = self._new()
        return self.add(ln(o, a, "n_" + o), *self.meta[a])

    def geglu(self, a, il):
        return self.add(geglu(self._new(), a, il), self.meta[a][0] // 2, self.meta[a][1])

    def attn(self, a, heads, c, kv=None):
        o = self._new()
        return self.add(attn(o, a, heads, c, kv=(f"k_{o}", f"v_{o}") if kv else None), c, self.meta[a][1])


# =============================================================================================== the exact-tier generator
def _exact_structure(seed: int):
    rng = random.Random(7919 * seed + 1)
    hw = EXACT_SHAPES[(seed // 8) % 5]
    img = hw[1] > 1
    cin = 4 if seed % 3 == 0 else rng.choice(EXACT_CH)
    k3 = 3 if img else 1
    b = _Builder(hw, cin)
    C1, C2 = rng.choice(EXACT_CH), rng.choice(EXACT_CH)
    a = b.conv("x", C1, ks=k3)
    mid = None
    tpl = seed % 8
    if tpl == 0:                                        # three consumers of a; c's residual is the first cotangent of b2 (hand-over)
        b2 = b.conv(a, C1)
        c = b.conv(a, C1, ks=k3, res=b2)
        cur = b.conv(a, C1, res=c)
    elif tpl == 1:                                      # a product whose residual is its own input
        cur = b.conv(a, C1, ks=k3, res=a)
    elif tpl == 2:                                      # a's cotangent: d first, then c's residual arrives second (launch_axpy)
        b2 = b.conv(a, C1)
        c = b.conv(b2, C1, ks=k3, res=a)
        d = b.conv(a, C2)
        cur = b.conv(b.concat(c, d), C1)
    elif tpl == 3:                                      # concat(a, a)
        cur = b.conv(b.concat(a, a), C2, ks=k3)
    elif tpl == 4:                                      # a pass seeded at m: s is no descendant of m -- an inactive op between src and dst, an inactive window
        mid = b.conv(a, C1)
        s = b.conv(a, C2)
        m2 = b.conv(mid, C1, ks=k3)
        cc = b.concat(m2, s) if seed % 16 < 8 else b.concat(s, m2)
        cur = b.conv(cc, C1)
    elif tpl == 5:                                      # a pass seeded at m: only the residual of the last product carries a tangent
        mid = b.conv(a, C1)
        s = b.conv(a, C2, ks=k3)
        m2 = b.conv(mid, C1)
        cur = b.conv(s, C1, res=m2)
    elif tpl == 6:
        if img:                                         # pool, product, upsample, residual from before the pool
            q = b.conv(b.resample(a, False), C1, ks=3)
            cur = b.conv(b.resample(q, True), C1, res=a)
        else:                                           # fused multi-name projection, then a row bias
            f = b.conv(a, 0, fused=(8, 16, 8))
            cur = b.conv(f, C1, rowbias=True)
    else:
        if img:                                         # stride 2 (pad 1 | pad 0), upsampling product, long skip
            d = b.conv(a, C2, ks=3, stride=2, pad=(seed // 8) % 2)
            u = b.conv(d, C1, ks=3, up=True)
            cur = b.conv(b.concat(u, a), C1)
        else:
            cur = b.conv(a, C1, rowbias=True, res=a)
    # random extension: products with links back to earlier buffers of the same shape, a fused projection, a row bias, a concat
    has_rb = any(s.get("rowbias") for s in b.steps)
    for _ in range(rng.randint(1, 2)):
        if len(b.steps) >= 8:
            break
        c, h = b.meta[cur]
        same = [n for n, (cc, hh) in b.meta.items() if hh == h and cc % 8 == 0 and n != "x"]
        r = rng.random()
        if r < 0.2 and len(same) > 1:
            other = rng.choice([n for n in same if n != cur])
            cur = b.conv(b.concat(cur, other), rng.choice(EXACT_CH), ks=rng.choice((1, k3)))
        elif r < 0.35:
            cur = b.conv(cur, 0, fused=(8, 16, 8))
        elif r < 0.5 and not has_rb:
            has_rb = True
            cur = b.conv(cur, rng.choice(EXACT_CH), ks=rng.choice((1, k3)), rowbias=True)
        else:
            co = rng.choice(EXACT_CH)
            cand = [n for n in same if b.meta[n][0] == co]
            cur = b.conv(cur, co, ks=rng.choice((1, k3)), res=rng.choice(cand) if cand and rng.random() < 0.7 else None)
    if seed % 4 == 1:                                   # cout = 4 at a tap: the adjoint runs on zero-padded transposed weights
        cur = b.conv(cur, 4, ks=k3)
    g = Graph(seed, "exact", hw, cin, b.steps, [], [], *((2, 2) if (seed // 4) % 2 == 0 else (1, 3)), meta=b.meta)
    if mid is None:                                     # a tap that is not the last op: any inner buffer the end depends on
        ups = sorted(g.upstream(cur) - {g.producer(cur)})
        cands = [b.steps[i]["out"] for i in ups if b.meta[b.steps[i]["out"]][0] % 8 == 0]
        mid = rng.choice(cands)
    g.taps = [mid, cur]
    g.pairs = [(mid, cur)]
    return g


def _sparse(gen, shape, nnz):
    """[rows, ...] with `nnz` entries of +-1 per row"""
    w = torch.zeros(shape)
    flat = w.reshape(shape[0], -1)
    for r in range(shape[0]):
        idx = torch.randperm(flat.shape[1], generator=gen)[:nnz]
        flat[r, idx] = torch.randint(0, 2, (nnz,), generator=gen).float() * 2 - 1
    return w


def _tern(gen, shape, keep=1.0):
    v = torch.randint(-1, 2, shape, generator=gen).float()
    return v if keep >= 1.0 else v * (torch.rand(shape, generator=gen) < keep).float()


def _draw_exact(g: Graph, attempt: int) -> None:
    gen = torch.Generator().manual_seed(1000003 * g.seed + attempt)
    nnz = 2 if attempt < 3 else 1
    keep = 1.0 if attempt < 6 else 0.5 if attempt < 12 else 0.2
    p = {}
    for s in g.steps:
        if kind(s) != "conv":
            continue
        ci = g.meta[s["src"]][0]
        for n, co, hb in names_of(s):
            p[n + ".weight"] = _sparse(gen, (co, ci) if s["ks"] == 1 else (co, ci, s["ks"], s["ks"]), nnz)
            if hb:
                p[n + ".bias"] = _tern(gen, (co,), 0.5)
        if s["rowbias"]:
            p["rb_" + s["out"] + ".weight"], p["rb_" + s["out"] + ".bias"] = _sparse(gen, (r8(s["cout"]), TEMB), 1), _tern(gen, (r8(s["cout"]),), 0.5)
    if any(kind(s) == "conv" and s["rowbias"] for s in g.steps):
        p["rbpad.weight"], p["rbpad.bias"] = _sparse(gen, (RB_PAD, TEMB), 1), _tern(gen, (RB_PAD,))
    g.params, g.attempt = p, attempt
    g.x = _tern(gen, g.shape("x", g.B))
    g.V = [_tern(gen, g.shape(src, g.nt), keep) for src, _ in g.passes]
    g.U = [_tern(gen, g.shape(dst, g.nt), keep) for _, dst in g.passes]
    g.Hsrc = {src: _tern(gen, g.shape(src, g.B)) for src, _ in g.pairs}


def pools(g: Graph) -> int:
    return sum(1 for s in g.steps if kind(s) == "resample" and not s["up"])


def exact_top(g: Graph) -> float:
    """largest magnitude x 4^P over every stored value of every pass (module docstring); inf if a derivative pass returns all zeros"""
    ref = reference(g, F32)
    if any(float(ref[k][p].abs().max()) == 0.0 for k in ("jvp", "vjp") for p in range(len(g.passes))):
        return float("inf")
    return max(float(m.max()) for m in magnitudes(g)) * 4.0 ** pools(g)


def check_exact_precondition(g: Graph) -> float:
    top = exact_top(g)
    assert top < 2.0 ** 8, f"seed {g.seed}: magnitude x 4^P = {top} is not below 2^8"
    q = 4.0 ** pools(g)
    ref = reference(g, F32)
    for k in ("primal", "jvp", "vjp", "from"):
        for key, v in (ref[k].items() if isinstance(ref[k], dict) else enumerate(ref[k])):
            assert torch.equal(v * q, (v * q).round()), f"seed {g.seed}: {k} {key} is no multiple of 4^-P"
            assert torch.equal(rnd(v, BF).double(), v), f"seed {g.seed}: {k} {key} is not exact in bf16"
    return top


def random_tape(seed: int, tier: str) -> Graph:
    """deterministic in (seed, tier); iterates as (steps, taps, pairs)"""
    if tier == "real":
        return _real_tape(seed)
    assert tier == "exact", tier
    g = _exact_structure(seed)
    for attempt in range(40):
        _draw_exact(g, attempt)
        if exact_top(g) < 2.0 ** 8:
            return g
    raise AssertionError(f"seed {seed}: no exact draw in 40 attempts")


# =============================================================================================== the real-tier generator
RECIPES = (("res", "attn"), ("res_sc", "cross"), ("tf", "res_sc"), ("attn", "res", "cross"), ("tf", "cross"), ("res", "res_sc", "attn", "res"),
           ("cross", "res"), ("tf", "attn"), ("res_sc", "attn", "cross"), ("res", "tf"), ("attn", "res_sc", "res"), ("tf", "res", "cross", "res_sc"))


def _groups(c: int) -> int:
    return 32 if c % 32 == 0 and c >= 256 else 8


def _heads(c: int) -> int:
    return 8 if c == 320 else c // 64                   # d = 40 (SD) or d = 64


def _motif(b: _Builder, m: str, h: str) -> str:
    c, hw = b.meta[h]
    if m in ("res", "res_sc"):                          # DDPM ResBlock: GN + SiLU, product with row bias, GN + SiLU, product with residual
        co = c if m == "res" else {320: 64, 64: 128, 128: 64}[c]
        n1 = b.gn(h, _groups(c), True)
        c1 = b.conv(n1, co, ks=3, rowbias=True)
        n2 = b.gn(c1, _groups(co), True)
        sc = b.conv(h, co) if co != c else h
        return b.conv(n2, co, ks=3, res=sc)
    if m == "attn":                                     # GN, fused q | k | v, self-attention, projection with residual
        n = b.gn(h, _groups(c), False)
        qkv = b.conv(n, 0, fused=(c, c, c))
        return b.conv(b.attn(qkv, _heads(c), c), c, res=h)
    if m == "cross":                                    # norm, to_q, attention on the 77-row context, to_out with residual (to_q / to_out private: foldable)
        n = b.ln(h) if c == 320 else b.gn(h, _groups(c), False)
        q = b.conv(n, c, bias=False)
        return b.conv(b.attn(q, _heads(c), c, kv=True), c, res=h)
    assert m == "tf" and c == 320 and hw[0] * hw[1] == 60
    z = b.ln(h)
    qkv = b.conv(z, 0, fused=(c, c, c), bias=False)
    h1 = b.conv(b.attn(qkv, 8, c), c, res=h)
    z = b.ln(h1)
    ff = b.conv(z, 8 * c, interleave=64)                # GEGLU_SOLE_INPUT: read by the GEGLU alone
    return b.conv(b.geglu(ff, 64), c, res=h1)


def _real_tape(seed: int) -> Graph:
    rng = random.Random(104729 * seed + 3)
    rec = RECIPES[seed % len(RECIPES)]
    tf = "tf" in rec
    hw = (6, 10) if tf else REAL_SHAPES[seed % 3]
    c0 = 320 if tf else 64
    assert not tf or all(m == "res" for m in rec[:rec.index("tf")]), "the transformer block runs at C = 320: what precedes it keeps the width"
    b = _Builder(hw, 4)
    h0 = h = b.conv("x", c0, ks=3)
    mode = seed % 3                                     # 0: long-skip concat; 1: a motif between a stride-2 and an upsampling product; 2: two motifs side by side
    taps, motifs = [], list(rec)
    i = 0
    while i < len(rec):
        m = rec[i]
        if i == 1:
            taps.append(h)                              # fan-out: the input of the second motif is a tap as well
        if mode == 1 and m in ("res", "res_sc") and hw != (4, 4) and "down" not in motifs:
            motifs.append("down")
            c = b.meta[h][0]
            d = b.conv(h, c, ks=3, stride=2, pad=rng.choice((0, 1)))
            d = _motif(b, m, d)
            u = b.conv(d, c, ks=3, up=True)
            h = b.conv(b.concat(u, h), b.meta[d][0])
        elif mode == 2 and i == 0 and len(rec) > 1 and rec[1] != "tf" and not (m == "res_sc"):
            motifs.append("side")
            h1, h2 = _motif(b, m, h), _motif(b, rec[1], h)
            h = b.conv(b.concat(h1, h2), b.meta[h2][0])
            i += 1
            if not taps:
                taps.append(h)
        else:
            h = _motif(b, m, h)
        i += 1
    if mode == 0 or "down" not in motifs and "side" not in motifs:
        motifs.append("skip")
        c = b.meta[h][0]
        h = b.conv(b.concat(h, h0), c, ks=3 if seed % 2 else 1)
    if len(taps) == 0 or taps[0] == h:
        taps = [h0]
    g = Graph(seed, "real", hw, 4, b.steps, [taps[0], h], [(taps[0], h)], *((2, 2) if seed % 2 == 0 else (1, 3)), meta=b.meta, motifs=motifs,
              ctx=CTX if "cross" in rec else None, t=1.0)
    gen = torch.Generator().manual_seed(15485863 * seed + 11)
    p = {}
    for s in g.steps:
        k = kind(s)
        if k in ("gn", "ln"):
            p[s["name"] + ".weight"], p[s["name"] + ".bias"] = affine(gen, g.meta[s["src"]][0])
        elif k == "attn" and s["kv"]:
            for n in s["kv"]:
                p[n + ".weight"] = torch.randn(s["c"], CTX[1], generator=gen) / math.sqrt(CTX[1])
        elif k == "conv":
            ci = g.meta[s["src"]][0]
            for n, co, hb in names_of(s):
                shape = (co, ci) if s["ks"] == 1 else (co, ci, s["ks"], s["ks"])
                p[n + ".weight"] = torch.randn(*shape, generator=gen) / math.sqrt(s["ks"] ** 2 * ci)
                if hb:
                    p[n + ".bias"] = 0.5 * torch.randn(co, generator=gen)
            if s["rowbias"]:
                co = r8(s["cout"])
                p["rb_" + s["out"] + ".weight"], p["rb_" + s["out"] + ".bias"] = torch.randn(co, TEMB, generator=gen) / 4.0, 0.5 * torch.randn(co, generator=gen)
    if any(kind(s) == "conv" and s["rowbias"] for s in g.steps):
        p["rbpad.weight"], p["rbpad.bias"] = torch.randn(RB_PAD, TEMB, generator=gen) / 4.0, torch.randn(RB_PAD, generator=gen)
    g.params = p
    scale = torch.tensor([1.0, 2.0])[:g.B].reshape(-1, 1, 1, 1)
    g.x = torch.randn(*g.shape("x", g.B), generator=gen) * scale
    if g.ctx:
        g.ctx_in = torch.randn(g.B, *CTX, generator=gen) * scale.reshape(-1, 1, 1)
    g.V = [torch.randn(*g.shape(src, g.nt), generator=gen) for src, _ in g.passes]
    g.U = [torch.randn(*g.shape(dst, g.nt), generator=gen) for _, dst in g.passes]
    g.Hsrc = {src: torch.randn(*g.shape(src, g.B), generator=gen) for src, _ in g.pairs}
    return g


_CORPUS: Dict[Tuple[str, int], Graph] = {}


def tape(tier: str, seed: int) -> Graph:
    """random_tape, built once per process (the generator redraws; the tests share the result and leave it unchanged)"""
    if (tier, seed) not in _CORPUS:
        _CORPUS[(tier, seed)] = random_tape(seed, tier)
    return _CORPUS[(tier, seed)]


# =============================================================================================== fp64 restatement
class _Store(torch.autograd.Function):
    """a buffer stored in the engine dtype: the value, its tangent and its cotangent are each rounded once"""

    @staticmethod
    def forward(x, dtype):
        return x.float().to(dtype).to(x.dtype)

    @staticmethod
    def setup_context(ctx, inputs, output):
        ctx.dt = inputs[1]

    @staticmethod
    def backward(ctx, gy):
        return gy.float().to(ctx.dt).to(gy.dtype), None

    @staticmethod
    def jvp(ctx, t, _):
        return t.float().to(ctx.dt).to(t.dtype)


def _rows(x):
    """[n, C, H, W] -> [n, HW, C]"""
    return x.flatten(2).transpose(1, 2)


def _img(r, hw):
    return r.transpose(1, 2).reshape(r.shape[0], r.shape[2], *hw)


def evaluate(g: Graph, dtype, x: torch.Tensor, ctx: Optional[torch.Tensor] = None, linear: bool = False, absolute: bool = False, store=None,
             override: Optional[Dict[str, torch.Tensor]] = None, cut=()) -> Dict[str, torch.Tensor]:
    """every buffer of the net on x [n, cin, H, W] (ctx [n, L, D]) in x's dtype.  Weights of products are the values the engine holds (rounded to
    `dtype`), biases and norm affines fp32.  linear: no bias / row bias (the tangent map of the exact tier).  absolute: weights, biases and the
    embedding by their absolute values (`magnitudes`).  store: round every stored buffer to that dtype.  override: buffers replaced by the given
    tensors (the seed of a between pass, the h of forward_from).  cut: (step, role) inputs that pass no derivative on, (step, "nores") residuals
    left out altogether (`drop`)."""
    A = (lambda t: t.abs()) if absolute else (lambda t: t)
    P = lambda n: A(g.params[n].to(x.dtype))
    Wt = lambda n: A(rnd(g.params[n + ".weight"], dtype).to(x.dtype))
    St = (lambda t: _Store.apply(t, store)) if store is not None else (lambda t: t)
    override = override or {}
    cut = set(cut)
    v = {"x": override.get("x", x)}
    n = x.shape[0]

    def take(k, role, name):
        return v[name].detach() if (k, role) in cut else v[name]

    for k, s in enumerate(g.steps):
        op, out = kind(s), s["out"]
        a = take(k, "src", s["src"])
        hw = g.meta[out][1]
        if op == "conv":
            y = _conv(s, a, torch.cat([Wt(nm) for nm, _, _ in names_of(s)], dim=0), None)
            if not linear:
                if any(hb for _, _, hb in names_of(s)):
                    bias = torch.cat([P(nm + ".bias") if hb else torch.zeros(co, dtype=x.dtype) for nm, co, hb in names_of(s)])
                    y = y + bias[None, :, None, None]
                if s["rowbias"]:
                    emb = A(temb_rows([g.t]).to(x.dtype))
                    rb = St(emb @ Wt("rb_" + out).T + P("rb_" + out + ".bias"))
                    y = y + rb[:, :s["cout"], None, None]
            if s["res"] and (k, "nores") not in cut:
                y = y + take(k, "res", s["res"])
            if s.get("interleave"):
                y = y[:, interleave_perm(s["cout"] // 2, s["interleave"])]
        elif op == "gn":
            y = _img(group_norm_ref(_rows(a), P(s["name"] + ".weight"), P(s["name"] + ".bias"), s["G"], s["eps"], s["silu"]), hw)
        elif op == "ln":
            y = _img(layer_norm_ref(_rows(a), P(s["name"] + ".weight"), P(s["name"] + ".bias"), s["eps"]), hw)
        elif op == "geglu":
            y = _img(geglu_ref(_rows(a), s["il"]), hw)
        elif op == "concat":
            y = torch.cat([a, take(k, "src2", s["src2"])], dim=1)
        elif op == "resample":
            y = F.interpolate(a, scale_factor=2, mode="nearest") if s["up"] else F.avg_pool2d(a, 2)
        elif op == "attn":
            c, H = s["c"], s["heads"]
            r = _rows(a)
            if s["kv"]:
                kv = St(ctx.to(x.dtype) @ torch.cat([Wt(nm) for nm in s["kv"]], dim=0).T)
                q, kk, vv = r, kv[..., :c], kv[..., c:]
            else:
                q, kk, vv = r[..., :c], r[..., c:2 * c], r[..., 2 * c:]
            sp = lambda t: t.reshape(n, t.shape[1], H, c // H).transpose(1, 2)
            o = torch.softmax(sp(q) @ sp(kk).transpose(-1, -2) / math.sqrt(c // H), dim=-1) @ sp(vv)
            y = _img(o.transpose(1, 2).reshape(n, -1, c), hw)
        else:
            raise ValueError(op)
        v[out] = override[out] if out in override else St(y)
    return v


def _rx(g, dtype):
    return rnd(g.x, dtype).double(), (rnd(g.ctx_in, dtype).double() if g.ctx else None)


def reference(g: Graph, dtype, store=None, drop=None) -> dict:
    """fp64: {"primal": {tap: O [B, ...]}, "jvp": [dO per pass], "vjp": [gX per pass], "forward": O at the last tap, "from": {(src, dst): O}}.
    Pass p runs from passes[p][0] to passes[p][1] with V[p] / U[p]; drop: a feature of `feature_instances` (see `drop`)."""
    x, ctx = _rx(g, dtype)
    cut, widen, by_j = [], None, False
    if drop is not None:
        if drop[0] in ("consumer", "residual"):
            cut = [(drop[1], drop[2])]
        elif drop[0] == "window":
            widen = drop[1:]
        elif drop[0] == "sample":
            by_j = True
    nores = [c for c in cut if c[1] == "nores"]
    out = {"primal": {}, "jvp": [], "vjp": [], "from": {}}
    with torch.no_grad():
        full = evaluate(g, dtype, x, ctx, store=store, cut=nores)
    out["primal"] = {t: full[t] for t in g.taps}
    out["forward"] = full[g.last]
    idx = torch.arange(g.nt).clamp(max=g.B - 1) if by_j else torch.arange(g.nt) // g.kps
    xs, cs = x[idx], (ctx[idx] if ctx is not None else None)
    tx = {}
    for p, (src, dst) in enumerate(g.passes):
        f = lambda h, src=src, dst=dst: evaluate(g, dtype, xs, cs, store=store, override={src: h}, cut=cut)[dst]
        base = full[src][idx]
        V, U = rnd(g.V[p], dtype).double(), rnd(g.U[p], dtype).double()
        _, dO = torch.func.jvp(f, (base,), (V,))
        if widen is not None and widen[0] == p:         # the inactive window keeps the tangent the x-seeded pass left there
            w = widen[1]
            if w not in tx:
                _, tx[w] = torch.func.jvp(lambda h: evaluate(g, dtype, h, cs, store=store)[w], (xs,), (rnd(g.V[0], dtype).double(),))
            f2 = lambda h, src=src, dst=dst: evaluate(g, dtype, xs, cs, store=store, override={src: base, w: h})[dst]
            dO = dO + torch.func.jvp(f2, (full[w][idx],), (tx[w],))[1]
        hs = base.clone().requires_grad_(True)
        y = f(hs)
        gx = torch.autograd.grad(y, hs, U)[0] if y.requires_grad else torch.zeros_like(hs)      # (a cut may sever the pass)
        out["jvp"].append(dO.detach())
        out["vjp"].append(gx.detach())
    with torch.no_grad():
        for src, dst in g.pairs:
            out["from"][(src, dst)] = evaluate(g, dtype, x, ctx, store=store, override={src: rnd(g.Hsrc[src], dtype).double()}, cut=nores)[dst]
    return out


def drop(g: Graph, dtype, feature, store=None) -> dict:
    """the reference with one bookkeeping contribution removed.  feature:
    ("consumer", step, role)  the derivative one consumer passes to the buffer it reads as `role` (src | src2 | res) is lost;
    ("residual", step, "nores")  the residual of that product is left out of every pass;
    ("window", pass, buffer)  the concat operand `buffer`, no descendant of the pass's src, keeps the tangent of the x-seeded pass;
    ("sample",)  tangent / cotangent j is linearised at sample min(j, B - 1) instead of j // kps."""
    return reference(g, dtype, store=store, drop=feature)


def feature_instances(g: Graph) -> List[tuple]:
    users: Dict[str, List[Tuple[int, str]]] = {}
    ups = g.upstream(g.last)
    for k, s in enumerate(g.steps):
        for role, b in inputs_of(s):
            if k in ups:
                users.setdefault(b, []).append((k, role))
    f = [("consumer", k, role) for b, u in users.items() if len(u) > 1 for k, role in u]
    f += [("residual", k, "nores") for k, s in enumerate(g.steps) if kind(s) == "conv" and s["res"] and k in ups]
    for p, (src, dst) in enumerate(g.passes[1:], 1):
        act, on = g.active(src)
        for k in g.upstream(dst):
            s = g.steps[k]
            if kind(s) == "concat" and on[k]:
                f += [("window", p, b) for b in (s["src"], s["src2"]) if b not in act and b != "x"]
    if g.B > 1 and g.tier == "real":                    # (a linear net has the same Jacobian at every sample)
        f.append(("sample",))
    return f


def affected(feature) -> List[str]:
    """the result kinds a dropped feature can change"""
    return {"consumer": ["jvp", "vjp"], "residual": ["primal", "jvp", "vjp"], "window": ["jvp"], "sample": ["jvp", "vjp"]}[feature[0]]


def magnitudes(g: Graph) -> List[torch.Tensor]:
    """exact tier: the same net on absolute values -- every buffer of the primal, of every tangent pass and (the sum of all contributions to its
    cotangent) of every adjoint pass, and of the seeded forward"""
    x = g.x.double().abs()
    m = list(evaluate(g, F32, x, absolute=True).values())
    z = torch.zeros(g.nt, *x.shape[1:], dtype=torch.float64)
    for p, (src, dst) in enumerate(g.passes):
        m += list(evaluate(g, F32, z, linear=True, absolute=True, override={src: g.V[p].double().abs()}).values())
        hs = torch.zeros(g.shape(src, g.nt), dtype=torch.float64, requires_grad=True)
        v = evaluate(g, F32, z, linear=True, absolute=True, override={src: hs})
        bufs = [t for t in v.values() if t.requires_grad]
        m += [t for t in torch.autograd.grad(v[dst], bufs, g.U[p].double().abs(), allow_unused=True) if t is not None]
    for src, dst in g.pairs:
        m += list(evaluate(g, F32, x, absolute=True, override={src: g.Hsrc[src].double().abs()}).values())
    return m


# =============================================================================================== census
def census(g: Graph) -> set:
    """the bookkeeping features a tape reaches (tests/test_graph_host.py asserts the corpus reaches every one)"""
    f = set(g.motifs)
    users: Dict[str, set] = {}
    for k, s in enumerate(g.steps):
        for _, b in inputs_of(s):
            users.setdefault(b, set()).add(k)
    f |= {"fan2" for u in users.values() if len(u) == 2} | {"fan3" for u in users.values() if len(u) >= 3}
    for s in g.steps:
        k = kind(s)
        if k == "conv":
            f.add("fused" if isinstance(s["name"], tuple) else "up" if s["up"] else f"s2p{s['pad']}" if s["stride"] == 2 else f"conv{s['ks']}")
            f |= {"rowbias"} if s["rowbias"] else set()
            f |= {"residual"} if s["res"] else set()
            f |= {"self_res"} if s["res"] and s["res"] == s["src"] else set()
        elif k == "concat":
            f.add("concat_aa" if s["src"] == s["src2"] else "concat")
        elif k == "resample":
            f.add("resample_up" if s["up"] else "resample_pool")
    f |= {"cin4"} if g.cin == 4 else set()
    f |= {"cout4_tap"} if any(g.meta[t][0] == 4 for t in g.taps) else set()
    f |= {"tap_mid"} if any(g.producer(t) != len(g.steps) - 1 for t in g.taps) else set()
    f |= {"hw60"} if g.hw == (6, 10) else set()
    for src, dst in g.passes:                           # the adjoint pass's first-write flags, restated: which route does each residual take
        act, on = g.active(src)
        ginit = {dst}
        for k in range(g.producer(dst), g.producer(src), -1):
            s = g.steps[k]
            if not on[k] or s["out"] not in ginit:
                continue
            for role, b in inputs_of(s):
                if b not in act:
                    continue
                if role == "res":
                    f.add("res_second" if b in ginit else "res_first")
                ginit.add(b)
        if src == "x":
            continue
        ups = g.upstream(dst)
        for k in range(g.producer(src) + 1, g.producer(dst) + 1):
            s = g.steps[k]
            if not on[k]:
                f.add("inactive_between")
            elif k in ups and kind(s) == "concat" and ((s["src"] in act) != (s["src2"] in act)):
                f.add("concat_inactive")
            elif k in ups and kind(s) == "conv" and s["res"] and s["src"] not in act:
                f.add("res_only_tangent")
    return f


EXACT_FEATURES = ("fan2", "fan3", "self_res", "res_first", "res_second", "concat_aa", "concat_inactive", "tap_mid", "inactive_between", "cin4",
                  "cout4_tap", "res_only_tangent", "conv1", "conv3", "s2p1", "s2p0", "up", "fused", "residual", "rowbias", "concat", "resample_pool",
                  "resample_up", "hw60")
REAL_MOTIFS = ("res", "res_sc", "attn", "tf", "cross")
REAL_COMPOSITIONS = ("skip", "down", "side")


# =============================================================================================== comparators
def to_rows(t: torch.Tensor) -> torch.Tensor:
    """[n, C, H, W] -> [n, HW, C], the rows of _norm_ref.row_errors"""
    return t.flatten(2).transpose(1, 2)


def errors(out: torch.Tensor, ref: torch.Tensor) -> Tuple[float, float]:
    """-> (largest row error of _norm_ref.row_errors, global relative error)"""
    out = out.detach().cpu().double().reshape(ref.shape)
    assert torch.isfinite(out).all(), "non-finite output"
    return float(row_errors(to_rows(out), to_rows(ref)).max()), float((out - ref).norm() / ref.norm().clamp_min(1e-300))


def flat_results(r: dict) -> Dict[str, torch.Tensor]:
    """one name per result of `reference` / `run_engine`"""
    o = {f"primal:{t}": v for t, v in r["primal"].items()}
    o.update({f"jvp:{p}": v for p, v in enumerate(r["jvp"])})
    o.update({f"vjp:{p}": v for p, v in enumerate(r["vjp"])})
    o["forward"] = r["forward"]
    o.update({f"from:{s}>{d}": v for (s, d), v in r["from"].items()})
    return o


def pass_of(name: str) -> str:
    """the (dtype, pass) class of a result's bound"""
    k = name.split(":")[0]
    return {"primal": "primal", "forward": "primal", "from": "primal", "jvp": "tangent", "vjp": "adjoint"}[k]


# (dtype, pass) -> largest row error of the real tier: twice the largest measured on an MI355X over the corpus and the arms of
# tests/test_gpu_graph.py (maxima in its docstring); dtype -> G, twice the largest ratio of the engine's global error to the ideal engine's
BOUNDS: Dict[Tuple[torch.dtype, str], float] = {
    (F32, "primal"): 1.4e-06, (F32, "tangent"): 2.2e-06, (F32, "adjoint"): 8.1e-06,
    (BF, "primal"): 2.0e-02, (BF, "tangent"): 3.6e-02, (BF, "adjoint"): 9.1e-02,
    (F16, "primal"): 2.5e-03, (F16, "tangent"): 3.5e-03, (F16, "adjoint"): 9.3e-03,
}
G: Dict[torch.dtype, float] = {F32: 19.1, BF: 3.3, F16: 3.5}


# =============================================================================================== the engine side
def build_tape(g: Graph, dtype, device):
    from diffusion_pullback_amd import lib as L
    from diffusion_pullback_amd.tape import Tape
    t = Tape(g.params, dtype, device)
    rb = any(kind(s) == "conv" and s["rowbias"] for s in g.steps)
    t.temb_in = t.buf(1, TEMB if rb else 8, L.BUF_SHARED)
    sh = t.shared_begin(t.temb_in, L.BUF_SHARED) if rb else None
    kv = None
    if g.ctx:
        t.ctx = t.buf(*g.ctx)
        kv = t.shared_begin(t.ctx, L.BUF_ACT)
    H, W = g.hw
    t.x = t.buf(H * W, r8(g.cin))
    if sh:
        t.shared_add(sh, "rbpad", RB_PAD)
    b = {"x": t.x}
    for s in g.steps:
        op, src = kind(s), b[s["src"]]
        hw = g.meta[s["src"]][1]
        if op == "conv":
            kw = {}
            if s["rowbias"]:
                kw = dict(rowbias=sh["out"], rowbias_off=t.shared_add(sh, "rb_" + s["out"], r8(s["cout"])))
            name = tuple(n for n, _, _ in s["name"]) if isinstance(s["name"], tuple) else s["name"]
            o = t.conv(name, src, hw, s["cout"], ks=s["ks"], stride=s["stride"], pad=s["pad"], upsample=s["up"], res=b[s["res"]] if s["res"] else -1,
                       interleave=s.get("interleave", 0), **kw)
        elif op == "gn":
            o = t.groupnorm(s["name"], src, s["G"], s["eps"], s["silu"])
        elif op == "ln":
            o = t.layernorm(s["name"], src, s["eps"])
        elif op == "geglu":
            o = t.geglu(src, s["il"])
        elif op == "concat":
            o = t.concat(src, b[s["src2"]])
        elif op == "resample":
            o = t.resample(src, hw, s["up"])
        elif op == "attn":
            c = s["c"]
            if s["kv"]:
                ko = t.shared_add(kv, tuple(s["kv"]), 2 * c)
                o = t.attention(src, kv["out"], kv["out"], s["heads"], c, (0, ko, ko + c))
            else:
                o = t.attention(src, src, src, s["heads"], c, (0, c, 2 * c))
        else:
            raise ValueError(op)
        b[s["out"]] = o
    for h in (kv, sh):
        if h is not None:
            t.shared_end(h)
    for name in g.taps:
        c, (h, w) = g.meta[name]
        t.tap(name, b[name], c, h, w)
    return t


def engine(g: Graph, dtype, device):
    from diffusion_pullback_amd.engine import Engine
    tp = build_tape(g, dtype, device)
    rb = any(kind(s) == "conv" and s["rowbias"] for s in g.steps)
    return Engine(tp, TEMB if rb else 8, False, True, g.cin, max_batch=g.B, max_tangents=g.nt)


def device_inputs(g: Graph, dtype, device) -> dict:
    d = lambda t: rnd(t, dtype).to(device)
    return dict(x=d(g.x), ctx=d(g.ctx_in) if g.ctx else None, V=[d(v) for v in g.V], U=[d(u) for u in g.U], H={k: d(v) for k, v in g.Hsrc.items()})


def run_engine(e, g: Graph, io: dict) -> Tuple[dict, Dict[str, int]]:
    """every call `reference` restates, in its layout (fp32 device tensors), and the launches of each"""
    out, n = {"primal": {}, "jvp": [], "vjp": [], "from": {}}, {}
    e.primal(io["x"], g.t, io["ctx"], g.last)
    n["primal"] = e.stats()[0]
    for t in g.taps:
        out["primal"][t] = e.read(t).clone()
    for p, (src, dst) in enumerate(g.passes):
        V, U = io["V"][p].reshape(g.nt, -1), io["U"][p].reshape(g.nt, -1)
        dO = e.jvp(dst, V) if src == "x" else e.jvp_between(src, dst, V)
        n[f"jvp:{p}"] = e.stats()[0]
        gx = e.vjp(dst, U) if src == "x" else e.vjp_between(src, dst, U)
        n[f"vjp:{p}"] = e.stats()[0]
        out["jvp"].append(dO.reshape(g.shape(dst, g.nt)).clone())
        out["vjp"].append(gx.reshape(g.shape(src, g.nt)).clone())
    out["forward"] = e.forward(io["x"], g.t, io["ctx"], g.last).clone()
    n["forward"] = e.stats()[0]
    for src, dst in g.pairs:
        out["from"][(src, dst)] = e.forward_from(io["x"], g.t, io["ctx"], src, io["H"][src], dst).clone()
        n[f"from:{src}>{dst}"] = e.stats()[0]
    return out, n
