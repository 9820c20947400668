"""Op-level attention checks: single-op tapes, an fp64 reference, crafted score patterns and a per-row comparator.

Layout convention of this module: activations are [batch, rows, channels] (the engine's NHWC rows); the engine's NCHW
interface sees them as [batch, channels, rows, 1].  Tangents / cotangents are [nt, rows, channels] with tangent j belonging to
sample j // kps, as in the engine.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import torch

FWD_THR = 4.0          # attn_fwd_kernel: a wave rescales once some query outgrows the stale max by more than 2^FWD_THR
SUB = 32               # keys per sub-tile of the flash forward's max update


def stage_keys(d: int) -> int:
    """keys per LDS stage of the fused kernels (FA<D>::BI)"""
    return 128 if d <= 80 else 64


def c2_of(d: int) -> float:
    """the kernel's fp32 log2-unit score factor scale * log2(e)"""
    scale = torch.tensor(1.0 / math.sqrt(d), dtype=torch.float32)      # 1.f / sqrtf((float)d)
    return float(scale * torch.tensor(1.44269504088896, dtype=torch.float32))


def rnd(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """the values the engine sees: fp32 input rounded to the engine dtype, back in fp32"""
    return t.float().to(dtype).float()


# =============================================================================================== single-op tapes
def _tape(dtype, device, rows: int, ch: int):
    from diffusion_pullback_amd import lib as L
    from diffusion_pullback_amd.tape import Tape
    t = Tape({}, dtype, device)
    t.temb_in = t.buf(1, 8, L.BUF_SHARED)
    t.x = t.buf(rows, ch)
    return t


def self_attention_tape(dtype, device, L: int, heads: int, d: int, causal: bool = False):
    """x [L][3C] = Q | K | V; one attention op over the three column windows"""
    C = heads * d
    t = _tape(dtype, device, L, 3 * C)
    o = t.attention(t.x, t.x, t.x, heads, C, (0, C, 2 * C), causal=causal)
    t.tap("o", o, C, L, 1)
    return t


def aliased_attention_tape(dtype, device, L: int, heads: int, d: int):
    """x [L][C] is q, k and v at once: the adjoint accumulates gQ + gK + gV into one window"""
    C = heads * d
    t = _tape(dtype, device, L, C)
    o = t.attention(t.x, t.x, t.x, heads, C, (0, 0, 0))
    t.tap("o", o, C, L, 1)
    return t


def cross_attention_tape(dtype, device, Lq: int, Lk: int, heads: int, d: int):
    """q = x [Lq][C]; k, v = the two column windows of the constant context [Lk][2C]"""
    C = heads * d
    t = _tape(dtype, device, Lq, C)
    t.ctx = t.buf(Lk, 2 * C)
    o = t.attention(t.x, t.ctx, t.ctx, heads, C, (0, 0, C))
    t.tap("o", o, C, Lq, 1)
    return t


def engine(tape, batch: int, tangents: int):
    from diffusion_pullback_amd.engine import Engine
    return Engine(tape, 8, False, True, tape.buffers[tape.x][1], max_batch=batch, max_tangents=tangents)


def to_nchw(x: torch.Tensor) -> torch.Tensor:
    """[B, rows, C] -> [B, C, rows, 1]"""
    return x.permute(0, 2, 1).unsqueeze(-1).contiguous()


def run_engine(e, x: torch.Tensor, ctx: Optional[torch.Tensor], V: Optional[torch.Tensor], U: Optional[torch.Tensor]):
    """x [B, L, Cx], ctx [B, Lk, 2C] or None, V [nt, L, Cx], U [nt, L, C] (device fp32) -> (O, dO, gX) as [., rows, ch] fp32"""
    dev = e.device
    e.primal(to_nchw(x).to(dev), 1.0, ctx, "o")
    O = e.read("o")[..., 0].permute(0, 2, 1)
    dO = gX = None
    if V is not None:
        dO = e.jvp("o", to_nchw(V).reshape(V.shape[0], -1)).reshape(V.shape[0], O.shape[2], -1).permute(0, 2, 1)
    if U is not None:
        gX = e.vjp("o", to_nchw(U).reshape(U.shape[0], -1)).reshape(U.shape[0], x.shape[2], -1).permute(0, 2, 1)
    return O, dO, gX


# =============================================================================================== fp64 reference
def _attend(q, k, v, scale, causal):
    s = scale * (q @ k.transpose(-1, -2))
    if causal:
        Lq, Lk = s.shape[-2:]
        mask = torch.ones(Lq, Lk, dtype=torch.bool, device=s.device).tril()
        s = s.masked_fill(~mask, float("-inf"))
    return torch.softmax(s, dim=-1) @ v


def reference(x: torch.Tensor, heads: int, d: int, offsets: Sequence[int], V: Optional[torch.Tensor] = None,
              U: Optional[torch.Tensor] = None, kps: int = 1, ctx: Optional[torch.Tensor] = None, causal: bool = False):
    """fp64 primal / tangent / adjoint of the op, by autograd (torch.func.jvp, torch.autograd.grad), chunked over heads.
    x [B, L, Cx] (already rounded to the engine dtype); ctx [B, Lk, Ck] for cross-attention (K / V windows of ctx, constant), else K / V
    are windows of x.  V [nt, L, Cx], U [nt, L, C]: tangent / cotangent j belongs to sample j // kps.  Returns (O [B,L,C], dO, gX) in fp64."""
    x = x.double()
    B, L, Cx = x.shape
    C = heads * d
    scale = 1.0 / math.sqrt(d)
    oq, ok, ov = offsets
    kv_src = ctx.double() if ctx is not None else None
    O = torch.empty(B, L, C, dtype=torch.float64, device=x.device)
    dO = torch.empty(V.shape[0], L, C, dtype=torch.float64, device=x.device) if V is not None else None
    gX = torch.zeros(U.shape[0], L, Cx, dtype=torch.float64, device=x.device) if U is not None else None
    for h in range(heads):
        def f(xx, kv=None):
            src = kv if kv is not None else xx
            q = xx[..., oq + h * d:oq + (h + 1) * d]
            k = src[..., ok + h * d:ok + (h + 1) * d]
            v = src[..., ov + h * d:ov + (h + 1) * d]
            return _attend(q, k, v, scale, causal)
        with torch.no_grad():
            O[..., h * d:(h + 1) * d] = f(x, kv_src)
        for tens, kind in ((V, "t"), (U, "a")):
            if tens is None:
                continue
            nt = tens.shape[0]
            idx = torch.arange(nt, device=x.device) // kps
            xs = x[idx]
            kvs = kv_src[idx] if kv_src is not None else None
            if kind == "t":
                _, out = torch.func.jvp(lambda xx: f(xx, kvs), (xs,), (tens.double(),))
                dO[..., h * d:(h + 1) * d] = out
            else:
                xs = xs.clone().requires_grad_(True)
                y = f(xs, kvs)
                (g,) = torch.autograd.grad(y, xs, tens.double()[..., h * d:(h + 1) * d])
                gX += g
    return O, dO, gX


def closed_form(q, k, v, dq, dk, dv, gO, scale):
    """closed-form JVP / VJP of one head (guards the autograd reference on a tiny case): returns O, dO, (gQ, gK, gV)"""
    P = torch.softmax(scale * q @ k.T, dim=-1)
    O = P @ v
    dS = scale * (dq @ k.T + q @ dk.T)
    dP = P * (dS - (P * dS).sum(-1, keepdim=True))
    dO = dP @ v + P @ dv
    gV = P.T @ gO
    gP = gO @ v.T
    gS = P * (gP - (P * gP).sum(-1, keepdim=True))
    return O, dO, (scale * gS @ k, scale * gS.T @ q, gV)


# =============================================================================================== crafted scores
PATTERNS = ("P1", "P2", "P3", "P4", "P5", "P6", "P7", "P8", "P9")
P6_GROWTH = 200.0      # log2 units: alpha = 2^-200 underflows to 0 in fp32


def _key_plan(pattern: str, L: int, d: int):
    """-> (b [L] log2-unit value of each key's controlled coordinate for a row with a_i = 1, landmark [L] bool: keys with no noise,
    a [32] per-lane row amplitudes of a wave)"""
    g = torch.Generator().manual_seed(sum(map(ord, pattern)) * 1000 + L + d)
    nsub = L // SUB
    bi = stage_keys(d)
    b = -1.0 - 2.0 * torch.rand(L, generator=g, dtype=torch.float64)     # background in [-3, -1]
    land = torch.zeros(L, dtype=torch.bool)
    a = torch.ones(32, dtype=torch.float64)
    late = (L // bi - 1) * bi + (bi // 2 if bi > SUB else 0)              # a sub-tile inside the last stage (not its first)
    late = min(late, L - SUB)

    def put(j, val):
        b[j] = val
        land[j] = True
    if pattern == "P1":
        put(5, 3.0)
        b[SUB:] -= 1.0
    elif pattern in ("P2", "P3", "P6"):
        put(3, 0.0)
        put(late + 7, {"P2": 3.9, "P3": 4.1, "P6": P6_GROWTH}[pattern])
    elif pattern == "P4":
        for t in range(min(nsub, 16)):
            put(t * SUB + (t * 5) % SUB, 3.9 * t)
    elif pattern == "P5":
        put(3, 0.0)
        put(late + 11, 4.1)
        a[:] = 0.5
        a[17] = 1.0                                                        # one lane of each wave crosses (4.1), the rest grow by 2.05
    elif pattern == "P7":
        b[:] = 0.0
    elif pattern == "P8":
        for j in sorted({j for j in (1, SUB + 2, bi + 9, L - SUB - 5, L // 2 + 3) if j < L}):
            put(j, 2.0)
    elif pattern == "P9":
        put(4, 0.0)
        put(L - 6, 6.0)
    else:
        raise ValueError(pattern)
    # softmax ignores a constant per row, the gradient of Q does not: sum_j gS_ij k_j with sum_j gS_ij = 0 amplifies the 16-bit rounding of gS
    # by |k| / spread(k) over the keys that carry the probability.  Shifting the scores so that the top key sits at 0 keeps the heavy keys'
    # k small (the growth steps are differences: unchanged)
    return b - b.max(), land, a


def crafted_qkv(pattern: str, L: int, heads: int, d: int, dtype: torch.dtype, seed: int = 0, noise: float = 0.02):
    """Q, K, V [L, heads*d] (fp32 holding dtype values) whose log2-unit scores c2 q.k follow `pattern` per query row.
    One coordinate per head (it moves with the head) carries the pattern; the others hold small noise (none on landmark keys).  A 16-bit
    key coordinate resolves a score of v log2 units only to v * 2^-9, too coarse for a 3.9 / 4.1 step on top of a staircase, so the key's
    value is split over two coordinates -- the rounded value and its rounded remainder -- that the query weights equally."""
    c2 = c2_of(d)
    b, land, a = _key_plan(pattern, L, d)
    g = torch.Generator().manual_seed(seed * 7919 + sum(map(ord, pattern)))
    C = heads * d
    Q = noise * torch.randn(L, C, generator=g, dtype=torch.float64)
    K = 0.5 * torch.randn(L, C, generator=g, dtype=torch.float64)
    V = torch.randn(L, C, generator=g, dtype=torch.float64)
    kc = (b / c2).to(dtype).double()
    kf = (b / c2 - kc).to(dtype).double()
    for h in range(heads):
        col, col2 = h * d + (7 * h + 3) % d, h * d + (7 * h + 4) % d
        K[land, h * d:(h + 1) * d] = 0.0
        Q[:, col] = Q[:, col2] = a.repeat(L // 32)
        K[:, col], K[:, col2] = kc, kf
        if pattern == "P8":                                                # exact ties: identical key rows
            K[land, h * d:(h + 1) * d] = K[land.nonzero()[0, 0], h * d:(h + 1) * d]
        if pattern == "P7":
            Q[:, h * d:(h + 1) * d] = 0.0
    return rnd(Q, dtype), rnd(K, dtype), rnd(V, dtype)


def growth(Q: torch.Tensor, K: torch.Tensor, d: int, head: int = 0) -> Dict[str, torch.Tensor]:
    """The flash forward's max bookkeeping of one head, replayed in fp64 with the kernel's fp32 c2: per wave of 32 queries and per 32-key
    sub-tile, step = max over the wave's lanes of (sub-tile max - stale max), rescale = whether the wave took the branch, lanes = how many lanes
    crossed the threshold.  Also returns the full log2 score matrix s2 [L, L]."""
    c2 = c2_of(d)
    q = Q[:, head * d:(head + 1) * d].double()
    k = K[:, head * d:(head + 1) * d].double()
    s2 = (q @ k.T) * c2
    L = s2.shape[0]
    nw, ns = L // 32, L // SUB
    mx = s2.reshape(nw, 32, ns, SUB).amax(-1)                              # [wave, lane, sub-tile]
    m = torch.full((nw, 32), float("-inf"), dtype=torch.float64)
    step = torch.empty(nw, ns, dtype=torch.float64)
    resc = torch.zeros(nw, ns, dtype=torch.bool)
    lanes = torch.zeros(nw, ns, dtype=torch.long)
    for t in range(ns):
        st = mx[:, :, t] - m
        step[:, t] = st.amax(1)
        cross = ~(st <= FWD_THR)
        lanes[:, t] = cross.sum(1)
        rw = cross.any(1)
        resc[:, t] = rw
        m = torch.where(rw[:, None], torch.maximum(m, mx[:, :, t]), m)
    return dict(step=step, rescale=resc, lanes=lanes, s2=s2)


def check_pattern(pattern: str, Q: torch.Tensor, K: torch.Tensor, d: int, heads: int) -> None:
    """asserts that the rounded inputs realise the growth sequence the pattern claims, for every head"""
    L = Q.shape[0]
    bi = stage_keys(d)
    ns = L // SUB
    for h in range(heads):
        gr = growth(Q, K, d, h)
        step, resc, lanes, s2 = gr["step"], gr["rescale"], gr["lanes"], gr["s2"]
        later = step[:, 1:]
        where = f"{pattern} d={d} L={L} head {h}"
        assert resc[:, 0].all(), where                                      # the first sub-tile always sets the max
        if pattern == "P1":
            assert (later <= 0).all() and not resc[:, 1:].any(), where
            assert (s2.argmax(1) < SUB).all(), where
        elif pattern == "P2":
            assert (later <= 3.95).all() and not resc[:, 1:].any(), where
            top = later.amax(1)
            assert (top >= 3.85).all(), (where, top.min())
            assert ((later.argmax(1) + 1) * SUB >= L - bi).all(), where     # in the last stage
        elif pattern == "P3":
            top = later.amax(1)
            assert ((top > FWD_THR) & (top <= 4.3)).all(), (where, top)
            assert (resc[:, 1:].sum(1) == 1).all(), where
            assert ((later.argmax(1) + 1) * SUB >= L - bi).all(), where
        elif pattern == "P4":
            n = min(ns, 16)
            assert (later <= 7.9).all(), where
            assert (resc[:, 1:n].sum(1) == (n - 1) // 2).all(), (where, resc[0, :n])
            assert resc[:, 2:n:2].all() and not resc[:, 1:n:2].any(), where   # every other step of the staircase
            assert not resc[:, n:].any(), where
        elif pattern == "P5":
            crossed = lanes[:, 1:].amax(1)
            assert (crossed == 1).all(), (where, crossed)                  # exactly one lane of every wave outgrows the stale max
            assert (resc[:, 1:].sum(1) == 1).all(), where
            assert ((later > FWD_THR) & (later <= 4.3)).any(1).all(), where
        elif pattern == "P6":
            assert (later.amax(1) >= 150).all(), where
            assert float(torch.tensor(-later.amax().item(), dtype=torch.float32).exp2()) == 0.0, where
        elif pattern == "P7":
            assert (s2 == s2[0, 0]).all(), where
        elif pattern == "P8":
            top = s2.amax(1, keepdim=True)
            hit = (s2 == top)
            assert (hit.sum(1) >= 3).all(), where
            cols = hit.nonzero()[:, 1]
            assert (cols // SUB).unique().numel() >= min(3, L // SUB) and (L <= bi or (cols // bi).unique().numel() >= 2), where
        elif pattern == "P9":
            assert (s2.argmax(1) >= L - SUB).all(), where
            assert (later.argmax(1) == ns - 2).all() and (later[:, -1] > 0).all(), where


# =============================================================================================== comparator
# (route family, engine dtype) -> {pass: (row bound, global bound)}: twice the largest error measured on an MI355X over the cases of the family
# (tests/test_gpu_attn_ops.py; maxima in its docstring).  BOUNDS: random Q, K, V; CRAFTED: the score patterns P1-P9, whose peaked rows make the
# adjoint's gS = P o (gP - D) a small difference of 16-bit quantities.
BOUNDS = {
    ("mat", torch.float32): {"primal": (4e-6, 2.1e-6), "tangent": (4e-6, 2.1e-6), "adjoint": (4e-6, 2.1e-6)},
    ("fused", torch.bfloat16): {"primal": (8.2e-3, 4.8e-3), "tangent": (3.8e-2, 1e-2), "adjoint": (3.2e-2, 7.5e-3)},
    ("fused", torch.float16): {"primal": (1e-3, 6e-4), "tangent": (5.4e-3, 1.25e-3), "adjoint": (4e-3, 9.2e-4)},
    ("mat", torch.bfloat16): {"primal": (2.9e-2, 9.4e-3), "tangent": (3.9e-2, 1.01e-2), "adjoint": (3.75e-2, 1.01e-2)},
    ("mat", torch.float16): {"primal": (3.9e-3, 1.17e-3), "tangent": (4.7e-3, 1.27e-3), "adjoint": (5e-3, 1.26e-3)},
    ("cross", torch.bfloat16): {"primal": (2.8e-2, 8.3e-3), "tangent": (9.3e-3, 4.9e-3), "adjoint": (1.01e-2, 4.9e-3)},
    ("cross", torch.float16): {"primal": (3.6e-3, 1.03e-3), "tangent": (1.15e-3, 6.1e-4), "adjoint": (1.22e-3, 6.1e-4)},
}
CRAFTED = {
    ("fused", torch.bfloat16): {"primal": (6.4e-3, 4.6e-3), "tangent": (5e-2, 1.7e-2), "adjoint": (0.21, 1.65e-2)},
    ("fused", torch.float16): {"primal": (9e-4, 6e-4), "tangent": (6.4e-3, 2.1e-3), "adjoint": (6.5e-2, 2.1e-3)},
    ("mat", torch.bfloat16): {"primal": (1.27e-2, 8.2e-3), "tangent": (2.1e-2, 1e-2), "adjoint": (0.13, 1e-2)},
    ("mat", torch.float16): {"primal": (1.55e-3, 1.01e-3), "tangent": (2.7e-3, 1.25e-3), "adjoint": (1.73e-2, 1.24e-3)},
}
# P4 (a +3.9 staircase: the top key keeps P ~ 0.93, its gS is 7 % of gP) in bf16: the fused adjoint, whose D = gO . O comes from the 16-bit O,
# reaches 0.22 on the gK row of that key (fp16: 0.03, the materialised path: 0.065)
P4_FUSED_BF16_ADJOINT = (0.44, 1.24e-2)


def row_errors(out: torch.Tensor, ref: torch.Tensor, d: int, tau: float = 0.05):
    """out, ref [T, rows, Ch] -> per-row errors [T, G, rows] (G = Ch / d column groups: heads, or q / k / v windows of heads):
    |d row| / (|ref row| + tau * rms), rms = the larger of the rms row norms of the (T, group) and of the whole of T -- a head whose cotangent
    vanishes analytically (one-hot probabilities: gS = P o (gP - D) = 0) has no scale of its own, only the 16-bit rounding of D = gO . O"""
    T, R, Ch = ref.shape
    o = out.double().reshape(T, R, Ch // d, d).permute(0, 2, 1, 3)
    r = ref.double().reshape(T, R, Ch // d, d).permute(0, 2, 1, 3)
    rn = r.norm(dim=-1)
    rms = torch.maximum(rn.pow(2).mean(-1, keepdim=True), rn.pow(2).mean((-1, -2), keepdim=True)).sqrt()
    return (o - r).norm(dim=-1) / (rn + tau * rms + 1e-300)


def compare(out: torch.Tensor, ref: torch.Tensor, d: int, row_bound: float, glob_bound: float, what: str = "",
            measured: Optional[dict] = None) -> float:
    """asserts finiteness, every row error <= row_bound and the global relative error <= glob_bound; returns the worst row error.
    A failure names the worst (tangent, group, row).  `measured`: dict collecting the maxima per label (for setting bounds)."""
    out = out.to(ref.device)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    assert torch.isfinite(out).all(), f"{what}: non-finite output ({(~torch.isfinite(out)).sum().item()} elements)"
    e = row_errors(out, ref, d)
    worst = float(e.max())
    t, g, r = [int(i) for i in torch.unravel_index(e.argmax(), e.shape)]
    glob = float((out.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))
    if measured is not None:
        m = measured.setdefault(what.split(" ")[0], [0.0, 0.0])
        m[0] = max(m[0], worst); m[1] = max(m[1], glob)
    assert worst <= row_bound, f"{what}: row error {worst:.3e} > {row_bound:.1e} at (tangent {t}, group {g}, row {r}); global {glob:.3e}"
    assert glob <= glob_bound, f"{what}: global relative error {glob:.3e} > {glob_bound:.1e}"
    return worst
