"""Op-level checks of the conv / linear product kernels (OP_CONV: csrc/gemm*.hip behind the tile table kGemmTiles of csrc/kernels.h): tiny tapes of one
or two `Tape.conv` ops on a fresh engine, an fp64 reference that does not share the kernels' im2col view, an exact (integer) and a real (Gaussian)
input tier, and elementwise comparators.  Modelled on tests/_norm_ref.py.

A case is a `Case`: an (H, W) image of `cin` channels and a list of `cv` steps.  `build_tape` turns it into an engine tape, `evaluate` restates it with
torch.nn.functional.conv2d in fp64 on the CPU: F.interpolate(mode="nearest") in front of the upsampling convolution, F.pad(x, (0, 1, 0, 1)) for the
pad = 0 stride-2 form (the rule of Tape.conv), a 1x1 kernel on an [rows, 1] image for plain rows.  The tangent is the same map without bias and row
bias, the adjoint is autograd of it.  Weights of the reference are the values the engine holds: the parameters rounded to the engine dtype (biases
stay fp32).  Layout: everything is NCHW as at the engine's boundary, x [B, C, H, W], V [nt, C, H, W], U [nt, Cout, Ho, Wo]; tangent j belongs to
sample j // kps.

Exact tier
----------
Inputs, weights, biases, residuals and seeds are small integers (x, V, U in [-3, 3]; W, b in [-2, 2]; the sinusoid of t = 0 is exactly 0 | 1), all
representable in bf16, fp16 and fp32.  Every product kernel accumulates in fp32, adds bias / row bias / residual / old value in fp32 and rounds once
(round to nearest even) to the engine dtype.  If S = |A| |W|^T + |b| + |row bias| + |res| + ... (the same net on absolute values, `magnitude`) stays
below 2^24 in every element, every partial sum in ANY order -- any K split, any MFMA-internal order -- is an integer below 2^24 and therefore exact in
fp32, so the engine's output must equal ref64.float().to(dtype) bit for bit (and intermediates stored in the engine dtype, being rounded integers
computed exactly, are reproduced by rounding the reference's intermediates: `evaluate(..., store=dtype)`).  `check_exact_precondition` asserts
S.max() < 2^24 and, for fp16, |ref|.max() < 65504 for every pass of a case.

Real tier: the derived bound
----------------------------
Inputs are Gaussians rounded to the engine dtype T with unit roundoff u_T (_norm_ref.UNIT: 2^-24, 2^-8, 2^-11); the reference is exact for these
inputs.  A product sums K_total terms in fp32 and applies at most 4 further fp32 additions (bias, row bias, residual, old value).  By the standard
forward bound of recursive summation in any order (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 4.2:
|fl(sum) - sum| <= gamma_{n-1} sum |terms|, gamma_n ~ n 2^-24) the fp32 value acc the kernel holds before its one rounding satisfies
    |acc - ref| <= (K_total + 4) 2^-24 S,
with S the absolute-value sum above; the MFMA's internal accumulation order and intermediate width are unspecified, which the factor 2 covers:
    E = 2 (K_total + 4) 2^-24 S.
The final rounding to T adds at most u_T |acc| <= u_T (|ref| + E).  Hence, per element,
    |got - ref| <= u_T (|ref| + E) + E.
Where the engine stores an intermediate in T on the way to the output -- the first consumer's output that the second takes as its residual, the first
adjoint product that the second accumulates onto, the cotangent of the upsampled image before launch_pool2x2_sum, the cotangent a residual is added
to by a separate kernel, the row-bias projection -- each such store is one more rounding of a value whose magnitude is at most S + E, so with r such
extra stores (`extra_roundings`) the bound is
    |got - ref| <= u_T (|ref| + E) + E + r u_T (S + E).
r = 0 for a single product, where this is the bound as stated first.  The row bias adds a term of its own: the engine evaluates the sinusoid in fp32
(argument t * f_i with f_i from expf, then sinf / cosf: absolute error at most 4 * 2^-24 (1 + |t| f_i)) and rounds it to T, the reference takes it
from the fp64 formula; the difference, at most d_i = u_T |emb_i| + 4 * 2^-24 (1 + |t| f_i) per entry, reaches the output as at most |W_rb| d
(`Case.temb_slack`), which is added to E.
A K sum carried in 16 bits, a double rounding of a split-K partial or a 16-bit path in an fp32 engine break this bound by orders of magnitude
(tests/test_product_ops_host.py proves the first on the CPU).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

from _norm_ref import BF, F16, F32, UNIT, rnd  # noqa: F401  (re-exported for the tests)

TEMB = 16          # width of the time-embedding buffer of the row-bias case ([sin | cos], half - 1 denominator)
RB_PAD = 8         # columns in front of the row-bias window inside the fused projection: the window's offset is not 0


def r8(c: int) -> int:
    return (c + 7) // 8 * 8


# =============================================================================================== cases
def cv(out, src, name, cout, ks=3, stride=1, pad=1, up=False, res=None, bias=True, rowbias=False):
    """one Tape.conv step.  name: a parameter name, or a tuple of (name, cout_i, has_bias) for a fused projection (cout = sum of the cout_i)"""
    return dict(out=out, src=src, name=name, cout=cout, ks=ks, stride=stride, pad=pad, up=up, res=res, bias=bias, rowbias=rowbias)


@dataclass
class Case:
    name: str
    hw: Tuple[int, int]
    cin: int
    steps: List[dict]
    note: str = ""
    t_real: Tuple[float, ...] = (1.0, 2.5)          # per-sample timesteps of the real tier (row-bias case); the exact tier runs t = 0
    tags: Tuple[str, ...] = field(default_factory=tuple)

    @property
    def plain(self) -> bool:
        return all(s["ks"] == 1 for s in self.steps)

    @property
    def rowbias(self) -> bool:
        return any(s["rowbias"] for s in self.steps)

    def out_hw(self, s=None) -> Tuple[int, int]:
        s = s or self.steps[-1]
        h, w = self.hw
        if s["ks"] == 1:
            return h, w
        if s["up"]:
            return 2 * h, 2 * w
        ks, st, pad = s["ks"], s["stride"], s["pad"]
        return ((h + 2 * pad - ks) // st + 1, (w + 2 * pad - ks) // st + 1) if pad else ((h + 1 - ks) // st + 1, (w + 1 - ks) // st + 1)

    def k_total(self, which: str) -> int:
        """K of all the products that reach the output in pass `which` (padded channel counts, as the kernels see them)"""
        k = sum(s["ks"] ** 2 * (r8(s["cout"]) if which == "adjoint" else r8(self.cin)) for s in self.steps)
        return k + (TEMB if self.rowbias and which == "primal" else 0)

    def extra_roundings(self, which: str) -> int:
        """stores of an intermediate in the engine dtype on the way to the output of pass `which` (module docstring)"""
        r = 0
        if which == "adjoint":
            r += len(self.steps) - 1                                   # the second product accumulates onto the stored first
            r += sum(1 for s in self.steps if s["up"])                 # the upsampled cotangent, then the 2x2 sum
            r += sum(1 for s in self.steps if s["res"] == "x")         # the product is stored, the residual's cotangent added by a separate kernel
        else:
            r += sum(1 for s in self.steps if s["res"] not in (None, "x"))   # the first consumer's stored output is the second's residual
            r += 1 if self.rowbias and which == "primal" else 0        # the row-bias projection
        return r


def _plain(name, rows, cin, cout, **kw):
    return Case(name, (rows, 1), cin, [cv("o", "x", "c", cout, ks=1, **kw)])


# The smallest shapes at which each edge exists (B = 2, kps = 2 unless a test says otherwise).
CASES: Dict[str, Case] = {c.name: c for c in [
    # ---- plain rows (ks = 1)
    _plain("rows40_72_200", 40, 72, 200),        # M = 80 smaller than the 128 / 256-row tiles (40 at B = 1: than every tile), K % 64 = K % 32 = 8, N % 64 = 8
    Case("rows300_320_320", (300, 1), 320, [cv("o", "x", "c", 320, ks=1, res="x")]),   # M = 600: 600 % 32 = 24, % 128 = 88; K = 320, N = 320: code 540
    _plain("rows264_328_264", 264, 328, 264),    # K % 64 = 8, N % 256 = 8: the 256-wide tiles 518 and 530
    _plain("rows24_8_13", 24, 8, 13),            # N % 8 != 0: scalar epilogue, padded output channels stay zero; K = 8 is less than one K tile
    Case("fused40_40_48", (40, 1), 40, [cv("o", "x", (("q", 16, True), ("k", 24, False), ("v", 8, True)), 48, ks=1)]),   # q | k | v, k without bias
    Case("rowbias24_16_40", (24, 1), 16, [cv("o", "x", "c", 40, ks=1, rowbias=True)]),   # 24 rows per sample: the sample boundary lies inside every tile
    # ---- 3x3, stride 1, pad 1
    Case("c3_16x8_64_72", (16, 8), 64, [cv("o", "x", "c", 72)]),       # hw = 128: two samples share a halo tile; forward halo-eligible, adjoint not (72 % 64)
    Case("c3_8x32_128_64", (8, 32), 128, [cv("o", "x", "c", 64)]),     # halo in both directions, 8-phase tile with gather
    Case("c3_12x20_40_40", (12, 20), 40, [cv("o", "x", "c", 40)]),     # non-square, no power of two, every K tile straddles taps; a split of 3 starts mid-tap
    # ---- stride 2
    Case("s2p1_16x12_72_136", (16, 12), 72, [cv("o", "x", "c", 136, stride=2)]),
    Case("s2p1_15x9_40_24", (15, 9), 40, [cv("o", "x", "c", 24, stride=2)]),          # odd size: last row / column border of the transposed gather
    Case("s2p0_16x12_40_72", (16, 12), 40, [cv("o", "x", "c", 72, stride=2, pad=0)]),  # asymmetric pad (0, 1, 0, 1)
    # ---- upsampling convolution
    Case("up_6x10_72_40", (6, 10), 72, [cv("o", "x", "c", 40, up=True)]),
    # ---- network ends
    Case("in_16x16_4_64", (16, 16), 4, [cv("o", "x", "c", 64)]),       # input channels padded to 8, x_channels = 4
    Case("out_16x16_64_4", (16, 16), 64, [cv("o", "x", "c", 4)]),      # N = 4; the adjoint runs on the zero-padded transposed weights
    # ---- two consumers: a = conv1(x), o = conv2(x, res = a): the second adjoint product accumulates, the residual hands its cotangent storage over
    Case("two_6x10_24_40", (6, 10), 24, [cv("a", "x", "c1", 40, ks=1), cv("o", "x", "c2", 40, res="a")]),
]}


def names_of(step) -> List[Tuple[str, int, bool]]:
    n = step["name"]
    return list(n) if isinstance(n, tuple) else [(n, step["cout"], step["bias"])]


# =============================================================================================== inputs
def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def make_params(case: Case, g: torch.Generator, tier: str, dtype) -> Dict[str, torch.Tensor]:
    """fp32 parameters, exactly representable in `dtype` for the exact tier; real tier: weights ~ randn / sqrt(K) (rounded by the engine), biases randn"""
    p = {}
    for s in case.steps:
        for n, co, hb in names_of(s):
            shape = (co, case.cin) if s["ks"] == 1 else (co, case.cin, s["ks"], s["ks"])
            if tier == "exact":
                p[n + ".weight"] = _ints(g, shape, -2, 2)
                if hb:
                    p[n + ".bias"] = _ints(g, (co,), -2, 2)
            else:
                p[n + ".weight"] = torch.randn(*shape, generator=g) / math.sqrt(s["ks"] ** 2 * case.cin)
                if hb:
                    p[n + ".bias"] = torch.randn(co, generator=g)
        if s["rowbias"]:
            for n, co in (("rbpad", RB_PAD), ("rb", r8(s["cout"]))):
                if tier == "exact":
                    p[n + ".weight"], p[n + ".bias"] = _ints(g, (co, TEMB), -2, 2), _ints(g, (co,), -2, 2)
                else:
                    p[n + ".weight"], p[n + ".bias"] = torch.randn(co, TEMB, generator=g) / 4.0, torch.randn(co, generator=g)
    return p


def make_inputs(case: Case, g: torch.Generator, tier: str, dtype, B: int, kps: int):
    """x [B, cin, H, W], V [B kps, cin, H, W], U [B kps, cout, Ho, Wo]: fp32 values representable in `dtype`"""
    (H, W), (Ho, Wo), co = case.hw, case.out_hw(), case.steps[-1]["cout"]
    shapes = ((B, case.cin, H, W), (B * kps, case.cin, H, W), (B * kps, co, Ho, Wo))
    if tier == "exact":
        return tuple(_ints(g, s, -3, 3) for s in shapes)
    return tuple(rnd(torch.randn(*s, generator=g), dtype) for s in shapes)


def temb_freqs() -> torch.Tensor:
    """the frequencies of oracle/unet_ddpm.py: timestep_embedding (fp32 exp, as there), in fp64"""
    half = TEMB // 2
    return torch.exp(torch.arange(half, dtype=torch.float32) * -(math.log(10000.0) / (half - 1))).double()


def temb_rows(ts) -> torch.Tensor:
    """[len(ts), TEMB] fp64: [sin | cos] of t * f_i, the formula of oracle/unet_ddpm.py: timestep_embedding evaluated in fp64"""
    ang = torch.tensor([float(t) for t in ts], dtype=torch.float64)[:, None] * temb_freqs()[None, :]
    return torch.cat([torch.sin(ang), torch.cos(ang)], dim=1)


# =============================================================================================== fp64 restatement
def _conv(step, x, w, case):
    ks = step["ks"]
    if ks == 1:
        return F.conv2d(x, w.reshape(w.shape[0], w.shape[1], 1, 1))
    if step["up"]:
        return F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)
    if step["pad"] == 0:
        return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=step["stride"])
    return F.conv2d(x, w, stride=step["stride"], padding=step["pad"])


def evaluate(case: Case, params, x: torch.Tensor, dtype, temb: Optional[torch.Tensor] = None, linear: bool = False, absolute: bool = False,
             store=None, wdtype=torch.float64) -> torch.Tensor:
    """the net on x [n, cin, H, W] (its dtype decides the arithmetic: fp64 for the reference).  temb [n, TEMB]: the time embedding of each row's sample
    (row-bias case).  linear: no bias / row bias (the tangent map).  absolute: every weight, bias and embedding by its absolute value (`magnitude`).
    store: round intermediates the engine stores in its dtype (the first consumer's output, the row-bias projection) to that dtype."""
    A = (lambda t: t.abs()) if absolute else (lambda t: t)
    Wt = lambda n: A(rnd(params[n + ".weight"], dtype).to(x.dtype))
    Bs = lambda n: A(params[n + ".bias"].to(x.dtype))
    v = {"x": x}
    for s in case.steps:
        assert s["src"] == "x", "the reference chains no product on a product (intermediate rounding would enter the K sum)"
        w = torch.cat([Wt(n) for n, _, _ in names_of(s)], dim=0)
        y = _conv(s, x, w, case)
        if not linear:
            b = torch.cat([Bs(n) if hb else torch.zeros(co, dtype=x.dtype) for n, co, hb in names_of(s)])
            y = y + b[None, :, None, None]
            if s["rowbias"]:
                rb = A(temb.to(x.dtype)) @ Wt("rb").T + Bs("rb")
                if store is not None:
                    rb = rnd(rb, store).to(x.dtype)
                y = y + rb[:, :s["cout"], None, None]
        if s["res"]:
            r = v[s["res"]]
            if store is not None and s["res"] != "x":
                r = rnd(r, store).to(x.dtype)
            y = y + r
        v[s["out"]] = y
    return v[case.steps[-1]["out"]]


def _sample_temb(case, ts, idx):
    return temb_rows(ts)[idx] if case.rowbias else None


def reference(case: Case, params, x, V, U, dtype, kps: int, ts, absolute: bool = False, store=None):
    """fp64 (O [B, ...], dO [nt, ...], gX [nt, cin, H, W]); ts: the B timesteps.  absolute: the absolute-value sums S of the three passes instead"""
    a = (lambda t: t.abs()) if absolute else (lambda t: t)
    x, V, U = a(x.double()), a(V.double()), a(U.double())
    B, nt = x.shape[0], V.shape[0]
    O = evaluate(case, params, x, dtype, _sample_temb(case, ts, torch.arange(B)), absolute=absolute, store=store)
    dO = evaluate(case, params, V, dtype, linear=True, absolute=absolute, store=store)
    v = torch.zeros_like(V).requires_grad_(True)
    (gX,) = torch.autograd.grad(evaluate(case, params, v, dtype, linear=True, absolute=absolute), v, U)
    return O, dO, gX.detach()


def magnitude(case, params, x, V, U, dtype, kps, ts):
    """S of the module docstring for the three passes: the same net on absolute values"""
    return reference(case, params, x, V, U, dtype, kps, ts, absolute=True)


def exact_reference(case, params, x, V, U, dtype, kps, ts):
    """exact tier: what the engine must return bit for bit -- the fp64 values (integers) rounded once to the engine dtype, as fp32.  Intermediates
    stored in the engine dtype are rounded integers as well; the adjoint's (products of integers below 2^24, exact in fp32) are reproduced by
    rounding each contribution where the engine stores it."""
    O, dO, _ = reference(case, params, x, V, U, dtype, kps, ts, store=dtype)
    U = U.double()
    g = None
    for s in reversed(case.steps):                     # the engine's order: the last op's adjoint first, the next accumulates onto the stored value
        if s["up"]:                                    # the cotangent of the upsampled image is stored, launch_pool2x2_sum adds its 2x2 windows
            H, W = case.hw
            one = Case(case.name, (2 * H, 2 * W), case.cin, [dict(s, res=None, out="o", up=False)])
            v = torch.zeros(V.shape[0], case.cin, 2 * H, 2 * W, dtype=torch.float64).requires_grad_(True)
            (c,) = torch.autograd.grad(evaluate(one, params, v, dtype, linear=True), v, U)
            c = F.avg_pool2d(rnd(c, dtype).double(), 2) * 4.0
        else:
            one = Case(case.name, case.hw, case.cin, [dict(s, res=None, out="o")])
            v = torch.zeros_like(V.double()).requires_grad_(True)
            (c,) = torch.autograd.grad(evaluate(one, params, v, dtype, linear=True), v, U)
        g = rnd(c if g is None else g + c, dtype).double()
        if s["res"] == "x":
            g = rnd(g + U, dtype).double()
    return rnd(O, dtype), rnd(dO, dtype), g.float()


def check_exact_precondition(case, params, x, V, U, dtype, kps, ts) -> float:
    """asserts S.max() < 2^24 for every pass and |ref|.max() < 65504 for fp16; returns the largest S"""
    S = magnitude(case, params, x, V, U, dtype, kps, ts)
    R = reference(case, params, x, V, U, dtype, kps, ts)
    top = max(float(s.max()) for s in S)
    assert top < 2.0 ** 24, f"{case.name}: absolute-value sum {top} is not below 2^24"
    if dtype == F16:
        big = max(float(r.abs().max()) for r in R)
        assert big < 65504.0, f"{case.name}: |ref| reaches {big}, beyond fp16"
    for r in R:
        assert torch.equal(r, r.round()), f"{case.name}: the exact-tier reference is not integral"
    return top


def temb_slack(case, params, dtype, ts, B) -> Optional[torch.Tensor]:
    """[B, cout]: |W_rb| d of the module docstring, the reach of the fp32-vs-fp64 sinusoid and of its rounding to the engine dtype"""
    if not case.rowbias:
        return None
    t = torch.tensor([abs(float(a)) for a in ts], dtype=torch.float64)[:, None]
    f = temb_freqs()[None, :]
    d = UNIT[dtype] * temb_rows(ts).abs() + torch.cat([4 * 2.0 ** -24 * (1 + t * f)] * 2, dim=1)
    co = case.steps[-1]["cout"]
    return (d @ rnd(params["rb.weight"], dtype).double().abs().T)[:, :co]


def real_bound(case, which: str, ref: torch.Tensor, S: torch.Tensor, dtype, slack: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the elementwise bound of the module docstring for pass `which` (primal | tangent | adjoint)"""
    u = UNIT[dtype]
    E = 2.0 * (case.k_total(which) + 4) * 2.0 ** -24 * S
    if slack is not None and which == "primal":
        E = E + slack[:, :, None, None]
    return u * (ref.abs() + E) + E + case.extra_roundings(which) * u * (S + E)


# =============================================================================================== comparators
def _where(idx, shape) -> str:
    n, c, y, x = [int(i) for i in torch.unravel_index(torch.as_tensor(idx), shape)]
    return f"(sample {n}, y {y}, x {x}, channel {c})"


def compare_exact(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    """every element of got [n, C, H, W] (fp32 from the engine) equals want bit for bit; a failure names the worst element"""
    got = got.detach().cpu().reshape(want.shape)
    if torch.equal(got, want):
        return
    d = (got.double() - want.double()).abs()
    d[~torch.isfinite(d)] = float("inf")
    i = int(d.argmax())
    bad = int((got != want).sum())
    raise AssertionError(f"{what}: {bad} of {want.numel()} elements differ; worst at {_where(i, want.shape)}: got {got.reshape(-1)[i].item()!r}, "
                         f"expected {want.reshape(-1)[i].item()!r}")


def compare_real(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, what: str, measured: Optional[dict] = None, key=None) -> float:
    """every element within its bound; returns (and records under `key`) the largest |got - ref| / bound"""
    got = got.detach().cpu().reshape(ref.shape).double()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    ratio = (got - ref).abs() / bound.clamp_min(1e-300)
    worst = float(ratio.max())
    if measured is not None:
        measured[key] = max(measured.get(key, 0.0), worst)
    if worst > 1.0:
        i = int(ratio.argmax())
        raise AssertionError(f"{what}: {int((ratio > 1).sum())} of {ref.numel()} elements beyond the bound; worst at {_where(i, ref.shape)}: got "
                             f"{got.reshape(-1)[i].item():.9g}, reference {ref.reshape(-1)[i].item():.9g}, bound {bound.reshape(-1)[i].item():.3e} "
                             f"({worst:.2f} x)")
    return worst


# =============================================================================================== the engine side
def build_tape(case: Case, params, dtype, device):
    from diffusion_pullback_amd import lib as L
    from diffusion_pullback_amd.tape import Tape
    t = Tape(params, dtype, device)
    H, W = case.hw
    t.temb_in = t.buf(1, TEMB if case.rowbias else 8, L.BUF_SHARED)
    sh = t.shared_begin(t.temb_in, L.BUF_SHARED) if case.rowbias else None
    t.x = t.buf(H * W, r8(case.cin))
    b = {"x": t.x}
    for s in case.steps:
        kw = {}
        if s["rowbias"]:
            t.shared_add(sh, "rbpad", RB_PAD)
            kw = dict(rowbias=sh["out"], rowbias_off=t.shared_add(sh, "rb", r8(s["cout"])))
            assert kw["rowbias_off"] == RB_PAD
        name = tuple(n for n, _, _ in s["name"]) if isinstance(s["name"], tuple) else s["name"]
        b[s["out"]] = t.conv(name, b[s["src"]], (H, W), s["cout"], ks=s["ks"], stride=s["stride"], pad=s["pad"], upsample=s["up"],
                             res=b[s["res"]] if s["res"] else -1, **kw)
    if sh is not None:
        t.shared_end(sh)
    last = case.steps[-1]
    Ho, Wo = case.out_hw()
    t.tap("o", b[last["out"]], last["cout"], Ho, Wo)
    return t


def engine(case: Case, tape, batch: int, tangents: int):
    from diffusion_pullback_amd.engine import Engine
    return Engine(tape, TEMB if case.rowbias else 8, False, True, case.cin, max_batch=batch, max_tangents=tangents)


def run_engine(e, x, V, U, ts):
    """-> (O, dO, gX) fp32 device tensors in the shapes of `reference`, and the launch counts of the three passes"""
    t = ts[0] if all(a == ts[0] for a in ts) else list(ts)
    e.primal(x, t, None, "o")
    n = [e.stats()[0]]
    O = e.read("o").clone()
    dO = e.jvp("o", V.reshape(V.shape[0], -1)).reshape(V.shape[0], *O.shape[1:]).clone()
    n.append(e.stats()[0])
    gX = e.vjp("o", U.reshape(U.shape[0], -1)).reshape(V.shape).clone()
    n.append(e.stats()[0])
    return (O, dO, gX), n


def read_padded(e, channels: int) -> torch.Tensor:
    """the primal tap with its padding channels: [B, channels, H, W]"""
    import ctypes as C
    from diffusion_pullback_amd import lib as L
    buf = e.tape.taps["o"]
    _, h, w = e.tape.tap_shape[buf]
    out = torch.empty(e.batch, channels, h, w, dtype=torch.float32, device=e.device)
    L.check(e.lib.dpb_read_buffer(e.h, buf, channels, C.c_void_p(out.data_ptr())))
    return out
