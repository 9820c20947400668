"""Every attention route at op level against an fp64 reference (tests/_attn_ref.py): single-op tapes with Q, K, V, the tangents and the
cotangents chosen exactly, per-row errors, and a proof of which kernels ran (engine.profile: kind 7 flash forward, 8 fused tangent with the
waves per block in `gather`, 9 fused adjoint with the route bits in `gather`, 10 one-launch cross-attention; the materialised path records
none of them).

Row error = |d row| / (|ref row| + 0.05 rms row norm of its (tangent, head)); rows are query rows of O / dO and rows of gQ, gK, gV per head.
Bounds (tests/_attn_ref.py BOUNDS / CRAFTED) are twice the largest error measured on an MI355X over all cases of a family.  Measured maxima,
row / global, primal | tangent | adjoint:
  random inputs
    fp32 materialised   1.6e-6 / 5.2e-7 | 2.0e-6 / 1.0e-6 | 1.8e-6 / 5.9e-7
    bf16 fused          4.1e-3 / 2.4e-3 | 1.9e-2 / 4.9e-3 | 1.6e-2 / 3.7e-3
    fp16 fused          5.0e-4 / 3.0e-4 | 2.7e-3 / 6.2e-4 | 2.0e-3 / 4.6e-4
    bf16 materialised   1.4e-2 / 4.7e-3 | 1.9e-2 / 5.1e-3 | 1.9e-2 / 5.0e-3
    fp16 materialised   1.9e-3 / 5.8e-4 | 2.3e-3 / 6.3e-4 | 2.5e-3 / 6.3e-4
    bf16 cross          1.4e-2 / 4.1e-3 | 4.6e-3 / 2.4e-3 | 5.0e-3 / 2.4e-3
    fp16 cross          1.8e-3 / 5.1e-4 | 5.7e-4 / 3.0e-4 | 6.1e-4 / 3.0e-4
  crafted score patterns P1-P9
    bf16 fused          3.8e-3 / 2.4e-3 | 2.5e-2 / 8.5e-3 | 1.1e-1 / 8.3e-3   (P4: 2.2e-1 / 2.0e-3, its own bound)
    fp16 fused          4.5e-4 / 2.9e-4 | 3.2e-3 / 1.1e-3 | 3.2e-2 / 1.0e-3
    bf16 materialised   6.3e-3 / 4.1e-3 | 1.0e-2 / 5.0e-3 | 6.5e-2 / 5.0e-3
    fp16 materialised   7.7e-4 / 5.1e-4 | 1.4e-3 / 6.2e-4 | 8.6e-3 / 6.2e-4
"""

import pytest
import torch

import _attn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
D16 = [pytest.param(BF, id="bf16"), pytest.param(F16, id="fp16")]

BOUNDS = R.BOUNDS


def _lib():
    from diffusion_pullback_amd import lib as L
    return L.load()


def _set(key: str, value: int):
    from diffusion_pullback_amd import lib as L
    L.check(_lib().dpb_debug_set(key.encode(), value))


def _profiled(e, tmp_path, fn):
    """runs fn() under engine.profile; returns (fn's result, [(kind, gather, Z)] of the attention brackets)"""
    e.profile(True)
    try:
        out = fn()
        path = str(tmp_path / "prof.csv")
        e.profile_dump(path)
    finally:
        e.profile(False)
    rows = []
    with open(path) as fh:
        next(fh)
        for line in fh:
            f = line.split(",")
            if int(f[1]) in (7, 8, 9, 10):
                rows.append((int(f[1]), int(f[2]), int(f[6])))
    return out, rows


def _gen(shape, dtype, g, scale=1.0):
    return R.rnd(scale * torch.randn(*shape, generator=g), dtype)


def run_case(tmp_path, family, dtype, kind, L, H, d, B=1, kps=2, patterns=None, Lk=77, seed=0, expect=None, passes=("primal", "tangent", "adjoint")):
    """One op on a fresh engine: primal, tangent and adjoint against the fp64 reference; `expect` maps a pass to the attention brackets it must
    record ([(kind, gather)], in order); returns the measured (row, global) maxima per pass."""
    g = torch.Generator().manual_seed(seed)
    C = H * d
    ctx = None
    if kind == "self":
        if patterns:
            x = torch.stack([torch.cat(R.crafted_qkv(patterns[b], L, H, d, dtype, seed=seed + b), dim=1) for b in range(B)])
            for b in range(B):
                R.check_pattern(patterns[b], x[b, :, :C], x[b, :, C:2 * C], d, H)
        else:
            x = _gen((B, L, 3 * C), dtype, g)
        tape = R.self_attention_tape(dtype, DEV, L, H, d)
        offs = (0, C, 2 * C)
    elif kind == "alias":
        x = _gen((B, L, C), dtype, g)
        tape = R.aliased_attention_tape(dtype, DEV, L, H, d)
        offs = (0, 0, 0)
    else:
        x = _gen((B, L, C), dtype, g)
        ctx = _gen((B, Lk, 2 * C), dtype, g)
        tape = R.cross_attention_tape(dtype, DEV, L, Lk, H, d)
        offs = (0, 0, C)
    nt = B * kps
    V = _gen((nt,) + tuple(x.shape[1:]), dtype, g)
    U = _gen((nt, L, C), dtype, g)
    e = R.engine(tape, B, nt)
    xd, Vd, Ud = x.to(DEV), V.to(DEV), U.to(DEV)
    ctxd = ctx.to(DEV) if ctx is not None else None
    ref = R.reference(xd, H, d, offs, Vd if "tangent" in passes else None, Ud if "adjoint" in passes else None, kps=kps, ctx=ctxd)
    bounds = dict((R.CRAFTED if patterns else BOUNDS)[(family, dtype)])
    if patterns and "P4" in patterns and (family, dtype) == ("fused", BF):
        bounds["adjoint"] = R.P4_FUSED_BF16_ADJOINT
    label = f"{family}/{kind} {str(dtype)[6:]} L={L}{'/' + str(Lk) if kind == 'cross' else ''} H={H} d={d} B={B} kps={kps} {patterns or ''}"
    got = {}
    (O, _, _), rp = _profiled(e, tmp_path, lambda: R.run_engine(e, xd, ctxd, None, None))
    got["primal"] = (O, rp, ref[0], d)
    if "tangent" in passes:
        dO, rt = _profiled(e, tmp_path, lambda: e.jvp("o", R.to_nchw(Vd).reshape(nt, -1)))
        got["tangent"] = (dO.reshape(nt, C, L).permute(0, 2, 1), rt, ref[1], d)
    if "adjoint" in passes:
        gX, ra = _profiled(e, tmp_path, lambda: e.vjp("o", R.to_nchw(Ud).reshape(nt, -1)))
        got["adjoint"] = (gX.reshape(nt, x.shape[2], L).permute(0, 2, 1), ra, ref[2], d)
    measured = {}
    for name, (out, rows, r, dd) in got.items():
        if expect is not None:
            seen = [(k, gth) for k, gth, _ in rows]
            assert seen == expect.get(name, []), f"{label} {name}: attention brackets {seen}, expected {expect.get(name, [])} (a silent route change)"
        rb, gb = bounds[name]
        errs = {}
        R.compare(out, r, dd, rb, gb, f"{name} {label}", errs)
        measured[name] = errs[name]
        print(f"ATTN-ERR {name} {label} row={errs[name][0]:.3e} glob={errs[name][1]:.3e}")
    del e
    return measured


def _fused_expect(waves, route):
    """the brackets of a fused self-attention layer: forward, tangent (its waves per block), adjoint (its route bits)"""
    return {"primal": [(7, 0)], "tangent": [(8, waves)], "adjoint": [(9, route)]}


def _waves(d, L, pairs):
    """att_block_waves of attn_fused.hip"""
    if d != 40 or L % 256:
        return 4 if d > 80 else 8
    return 8 if ((L // 256) * pairs) % 256 == 0 else 4


# =============================================================================================== fp32: materialised path, tight bound
@pytest.mark.parametrize("d", [40, 64, 80, 160])
def test_fp32_materialised_self_attention(tmp_path, d):
    for L in (64, 200, 256, 1024):
        run_case(tmp_path, "mat", F32, "self", L, 2, d, B=2, kps=2, seed=L + d, expect={})


def test_fp32_materialised_aliased_and_cross(tmp_path):
    run_case(tmp_path, "mat", F32, "alias", 200, 2, 40, B=2, kps=2, seed=1, expect={})
    run_case(tmp_path, "mat", F32, "alias", 256, 5, 64, B=1, kps=3, seed=2, expect={})
    run_case(tmp_path, "mat", F32, "cross", 256, 2, 64, B=2, kps=2, Lk=77, seed=3, expect={})


@pytest.mark.parametrize("dtype", [F32, BF, F16], ids=["fp32", "bf16", "fp16"])
def test_causal_text_encoder_attention(tmp_path, dtype):
    """L = 77, 12 heads of 64 (CLIP text encoder), primal only; row i does not see keys after i, bit for bit"""
    g = torch.Generator().manual_seed(77)
    L, H, d = 77, 12, 64
    C = H * d
    x = _gen((2, L, 3 * C), dtype, g)
    e = R.engine(R.self_attention_tape(dtype, DEV, L, H, d, causal=True), 2, 1)
    (O, _, _), rows = _profiled(e, tmp_path, lambda: R.run_engine(e, x.to(DEV), None, None, None))
    assert rows == [], rows                                                # materialised softmax (the fused kernels have no mask)
    ref = R.reference(x.to(DEV), H, d, (0, C, 2 * C), causal=True)[0]
    rb, gb = BOUNDS[("mat", dtype)]["primal"]
    errs = {}
    R.compare(O, ref, d, rb, gb, f"primal causal {dtype}", errs)
    print(f"ATTN-ERR primal causal {str(dtype)[6:]} row={errs['primal'][0]:.3e} glob={errs['primal'][1]:.3e}")
    for i in (0, 40, 75):
        x2 = x.clone()
        x2[:, i + 1:, C:] = _gen((2, L - i - 1, 2 * C), dtype, g, 3.0)    # keys and values after i
        O2 = R.run_engine(e, x2.to(DEV), None, None, None)[0]
        assert torch.equal(O2[:, :i + 1], O[:, :i + 1]), i
        assert not torch.equal(O2[:, i + 1:], O[:, i + 1:]), i


# =============================================================================================== 16 bit: fused self-attention
@pytest.mark.parametrize("dtype", D16)
def test_fused_d40_lengths_waves_and_adjoint_routes(tmp_path, dtype):
    H, d = 8, 40
    try:
        for L, B, kps, shared, route in [(256, 1, 5, 2, 3),       # 4-wave tangent (40 pairs)
                                         (1024, 1, 8, 2, 3),      # 8-wave tangent (4 x 64 pairs = 256)
                                         (1024, 2, 5, 2, 3),      # two samples, 4-wave tangent
                                         (1024, 1, 7, 2, 3),      # ragged cotangent group (5 + 2)
                                         (1024, 1, 10, 2, 3),     # two full cotangent groups
                                         (1024, 1, 3, 2, 1),      # kps < 4: no shared-P key-major kernel
                                         (1024, 1, 5, 0, 1),      # attn_shared = 0
                                         (4096, 1, 2, 2, 1),      # 8-wave tangent (16 x 16 pairs)
                                         (4096, 1, 5, 2, 3)]:     # 4-wave tangent
            _set("attn_shared", shared)
            nt = B * kps
            run_case(tmp_path, "fused", dtype, "self", L, H, d, B=B, kps=kps, seed=L + kps,
                     expect=_fused_expect(_waves(d, L, nt * H), route))
    finally:
        _set("attn_shared", 2)


@pytest.mark.parametrize("dtype", D16)
def test_fused_other_head_dims(tmp_path, dtype):
    try:
        for shared, route in ((0, 0), (6, 3)):                   # d = 64 (5 heads at C = 320): per-cotangent kernels, then both shared-P kernels
            _set("attn_shared", shared)
            run_case(tmp_path, "fused", dtype, "self", 1024, 5, 64, B=1, kps=5, seed=64 + shared, expect=_fused_expect(8, route))
    finally:
        _set("attn_shared", 2)
    run_case(tmp_path, "fused", dtype, "self", 1024, 4, 80, B=1, kps=3, seed=80, expect=_fused_expect(8, 0))
    run_case(tmp_path, "fused", dtype, "self", 256, 2, 160, B=2, kps=2, seed=160, expect=_fused_expect(4, 0))
    run_case(tmp_path, "fused", dtype, "self", 64, 2, 160, B=1, kps=3, seed=161, expect=_fused_expect(4, 0))


@pytest.mark.parametrize("dtype", D16)
def test_fused_aliased_window_accumulates_all_three_cotangents(tmp_path, dtype):
    """q = k = v: gQ, gK and gV land in ONE window; the key-major kernels write gK + gV once"""
    try:
        for shared, route in ((2, 3), (0, 1)):
            _set("attn_shared", shared)
            run_case(tmp_path, "fused", dtype, "alias", 256, 8, 40, B=1, kps=5, seed=11, expect=_fused_expect(4, route))
    finally:
        _set("attn_shared", 2)
    run_case(tmp_path, "fused", dtype, "alias", 256, 5, 64, B=2, kps=2, seed=12, expect=_fused_expect(8, 0))


@pytest.mark.parametrize("dtype", D16)
@pytest.mark.parametrize("L", [1024, 4096])
def test_fused_d40_crafted_score_patterns(tmp_path, dtype, L):
    """P1-P9 (tests/_attn_ref.py): the deferred rescale of the flash forward at and around its threshold, alpha underflow, ties, flat rows"""
    H, d = 8, 40
    for i, p in enumerate(R.PATTERNS):
        run_case(tmp_path, "fused", dtype, "self", L, H, d, B=1, kps=2, patterns=[p], seed=i,
                 expect=_fused_expect(_waves(d, L, 2 * H), 1))
    run_case(tmp_path, "fused", dtype, "self", L, H, d, B=2, kps=5, patterns=["P3", "P5"], seed=20,     # two samples, two patterns
             expect=_fused_expect(_waves(d, L, 10 * H), 3))


@pytest.mark.parametrize("dtype", D16)
def test_fused_d80_d160_threshold_patterns(tmp_path, dtype):
    for p in ("P2", "P3", "P5"):
        run_case(tmp_path, "fused", dtype, "self", 1024, 4, 80, B=1, kps=2, patterns=[p], seed=3, expect=_fused_expect(8, 0))
        run_case(tmp_path, "fused", dtype, "self", 256, 2, 160, B=1, kps=2, patterns=[p], seed=4, expect=_fused_expect(4, 0))
        run_case(tmp_path, "fused", dtype, "self", 64, 2, 160, B=1, kps=2, patterns=[p], seed=5, expect=_fused_expect(4, 0))


# =============================================================================================== 16 bit: materialised path
@pytest.mark.parametrize("dtype", D16)
def test_materialised_16bit_same_shapes(tmp_path, dtype, monkeypatch):
    """DPB_FUSED_ATTN_MIN_L (read when the engine is created) sends the fused shapes back to GEMM + softmax + GEMM; scores are stored in 16 bit"""
    monkeypatch.setenv("DPB_FUSED_ATTN_MIN_L", "1000000")
    for L, H, d, kps in [(256, 8, 40, 5), (1024, 8, 40, 3), (4096, 8, 40, 2), (1024, 5, 64, 5), (1024, 4, 80, 3), (256, 2, 160, 2), (64, 2, 160, 3)]:
        run_case(tmp_path, "mat", dtype, "self", L, H, d, B=1, kps=kps, seed=L + d, expect={})
    run_case(tmp_path, "mat", dtype, "alias", 256, 8, 40, B=2, kps=2, seed=9, expect={})
    for i, p in enumerate(R.PATTERNS):
        if p != "P6":                                             # a 16-bit score of 200 log2 units is off by 2^-9 of itself
            run_case(tmp_path, "mat", dtype, "self", 1024, 8, 40, B=1, kps=2, patterns=[p], seed=i, expect={})


# =============================================================================================== 16 bit: cross-attention
@pytest.mark.parametrize("dtype", D16)
@pytest.mark.parametrize("d", [40, 64, 80, 160])
def test_cross_attention_one_launch_kernel(tmp_path, dtype, d):
    """constant K / V of a 77- or 96-key context (XKEYS = 96); Lq 64 and 96 run fewer than 4 waves per block; the primal with the one-launch
    kernel (cross_primal = 1) and on the materialised path (0)"""
    H = 320 // d if d != 160 else 2
    try:
        for Lq in (64, 96, 256, 1024):
            for Lk in (77, 96):
                for cp in (1, 0):
                    _set("cross_primal", cp)
                    run_case(tmp_path, "cross", dtype, "cross", Lq, H, d, B=2, kps=2, Lk=Lk, seed=Lq + Lk + d,
                             passes=("primal", "tangent", "adjoint") if cp else ("primal",),
                             expect={"primal": [(10, 2)] if cp else [], "tangent": [(10, 0)], "adjoint": [(10, 1)]})
    finally:
        _set("cross_primal", 1)
