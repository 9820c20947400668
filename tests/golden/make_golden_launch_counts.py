"""Records dpb_engine_stats -- (launches, gemm flops, gemm bytes) -- after every pass of a set of tiny tapes -> tests/golden/launch_counts.json.

The fixture pins what the engine reports per pass across refactors of the accounting: generate it ONCE, on a GPU, from a build of the commit whose
numbers are to be kept

    DPB_LIB=/path/to/that/libdpb.so python tests/golden/make_golden_launch_counts.py <commit hash>

and tests/test_gpu_launch_counts.py replays the same tapes (GROUPS below is shared by the generator and the test) on the library under test, entry
for entry.  An entry is "<group>/<case>": the list of [launches, flops, gbytes] triples of the case's passes, in the order the case runs them.

The tapes are the tiny nets of the op-level tests: the step nets of tests/_norm_ref.py, the single-op attention tapes of tests/_attn_ref.py, the tiny
SD and DDPM U-Nets of tests/test_gpu_hshift.py / test_gpu_decoder.py and a one-level 320-channel SD net as in tests/test_gpu_edge.py.  Batch 2, two
directions per sample (K), bf16 plus an fp32 pass per op kind.  Launch counts do not depend on the values, so inputs are plain seeded noise.
"""
import json
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(HERE, "launch_counts.json")
DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
NAME = {BF: "bf16", F32: "fp32"}
B, K = 2, 2
NT = B * K


def _L():
    from diffusion_pullback_amd import lib as L
    return L, L.load()


class _switches:
    """dpb_debug_set switches for the duration of a block, then back to their defaults.  DEFAULT is what the library starts with when no DPB_*
    environment variable overrides a switch: record() refuses to run otherwise, so the reset puts back the state the process started in."""
    DEFAULT = {"lazy_reduce": 1, "gn_deterministic": 1, "ln_fuse": 0, "geglu_fwd": 1, "cross_primal": 1, "gemm_tile": 0, "gemm_splitk": 0,
               "graph_iterate": 0}

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        L, lib = _L()
        for k, v in self.kv.items():
            L.check(lib.dpb_debug_set(k.encode(), v))

    def __exit__(self, *exc):
        L, lib = _L()
        for k in self.kv:
            L.check(lib.dpb_debug_set(k.encode(), self.DEFAULT[k]))


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _stat(e):
    n, f, b = e.stats()
    return [int(n), float(f), float(b)]


def _three(e, x, ctx, tap, n_out, passes=3):
    """primal, tangent, adjoint of the encoder entry points (passes = 1: primal only)"""
    e.primal(x, 1.0, ctx, tap)
    out = [_stat(e)]
    if passes == 1:
        return out
    e.jvp(tap, _rand(NT, e.n_in, seed=1))
    out.append(_stat(e))
    e.vjp(tap, _rand(NT, n_out, seed=2))
    out.append(_stat(e))
    return out


# ================================================================================================ step nets (tests/_norm_ref.py)
def _linear_params(name, cout, cin):
    g = torch.Generator().manual_seed(cout + cin)
    return {name + ".weight": torch.randn(cout, cin, generator=g) / math.sqrt(cin), name + ".bias": 0.5 * torch.randn(cout, generator=g)}


def _step_net(steps, params, dtype, rows, C, passes=3, forward_only=False):
    import _norm_ref as R
    tape = R.build_tape(steps, params, dtype, DEV, rows, C)
    e = R.engine(tape, B, NT)
    x = R.to_nchw(_rand(B, rows, C))
    if forward_only:
        e.forward(x, 1.0, None, "o")
        return [_stat(e)]
    return _three(e, x, None, "o", e.tap_numel("o"), passes)


def group_norm_ops():
    import _norm_ref as R
    out = {}
    g = torch.Generator().manual_seed(0)
    for dtype in (BF, F32):
        dn = NAME[dtype]
        # GroupNorm: one-launch kernel, two passes (the apply pass reduces), two passes + gn_reduce_kernel; fixed-order and atomic statistics
        for C, HW in ((320, 64), (320, 409), (32, 2056)):
            for det in (1, 0):
                with _switches(gn_deterministic=det):
                    out[f"gn C={C} HW={HW} det={det} {dn}"] = _step_net([R.gn("o", "x", "n", 32, 1e-5, True)], R.norm_params(g, ["n"], C), dtype, HW, C)
        out[f"ln C=320 rows=77 {dn}"] = _step_net([R.ln("o", "x", "n")], R.norm_params(g, ["n"], 320), dtype, 77, 320)
        out[f"geglu F=64 {dn}"] = _step_net([R.geglu("o", "x", 0)], {}, dtype, 77, 128)
        out[f"geglu F=64 forward {dn}"] = _step_net([R.geglu("o", "x", 0)], {}, dtype, 77, 128, forward_only=True)
        for fn in ("silu", "quick_gelu", "gelu"):
            out[f"{fn} {dn}"] = _step_net([R.unary("o", "x", fn)], {}, dtype, 77, 40, passes=1)
        out[f"concat(x, x) {dn}"] = _step_net([R.concat("o", "x", "x")], {}, dtype, 8, 64)
        out[f"linear 64->64 {dn}"] = _step_net([R.linear("o", "x", "p", 64)], _linear_params("p", 64, 64), dtype, 64, 64)
        # residual of a product: its first cotangent takes the product's storage (r has one reader), a later one is copied (x is read twice more)
        p = {**_linear_params("pa", 64, 64), **_linear_params("pb", 64, 64)}
        out[f"residual swap {dn}"] = _step_net([R.linear("r", "x", "pa", 64), R.linear("o", "x", "pb", 64, res="r")], p, dtype, 64, 64)
        out[f"residual copy {dn}"] = _step_net([R.linear("r", "x", "pa", 64), R.linear("c", "x", "pb", 64, res="x"), R.linear("o", "c", "pa", 64, res="r")],
                                               p, dtype, 64, 64)
    return out


def group_split_k():
    """a forced split: the reduction deferred to a GroupNorm / a LayerNorm, flushed because the next op is no norm; lazy_reduce 0 and 1"""
    import _norm_ref as R
    out = {}
    g = torch.Generator().manual_seed(1)
    nets = {
        "gn": ([R.linear("h", "x", "p1", 320), R.gn("z", "h", "n", 32, 1e-5, True), R.linear("o", "z", "p2", 2560)], 2560),
        "ln": ([R.linear("h", "x", "p1", 320), R.ln("z", "h", "n"), R.linear("o", "z", "p2", 1280)], 1280),
        "flush": ([R.linear("h", "x", "p1", 320), R.linear("o", "h", "p2", 1280)], 1280),
    }
    for dtype in (BF, F32):
        for name, (steps, Kc) in nets.items():
            params = {**R.norm_params(g, ["n"], 320), **_linear_params("p1", 320, Kc), **_linear_params("p2", Kc, 320)}
            for lazy in (1, 0):
                with _switches(gemm_tile=64, gemm_splitk=4, lazy_reduce=lazy):
                    out[f"{name} K={Kc}->320 splitk=4 lazy={lazy} {NAME[dtype]}"] = _step_net(steps, params, dtype, 64, Kc)
    return out


# ================================================================================================ attention tapes (tests/_attn_ref.py)
def group_attention():
    import _attn_ref as A
    out = {}

    def run(tape, Cx, L, ctx):
        e = A.engine(tape, B, NT)
        return _three(e, A.to_nchw(_rand(B, L, Cx)), ctx, "o", e.tap_numel("o"))

    for dtype in (BF, F32):
        dn = NAME[dtype]
        out[f"self L=64 d=40 materialised {dn}"] = run(A.self_attention_tape(dtype, DEV, 64, 2, 40), 240, 64, None)          # kv_const false
        for cp in (1, 0):                                                                                                   # kv_const true, 77 context rows
            with _switches(cross_primal=cp):
                out[f"cross Lq=64 Lk=77 d=40 cross_primal={cp} {dn}"] = run(A.cross_attention_tape(dtype, DEV, 64, 77, 2, 40), 80, 64, _rand(B, 77, 160, seed=3))
    out["self L=64 d=160 fused bf16"] = run(A.self_attention_tape(BF, DEV, 64, 1, 160), 480, 64, None)
    out["aliased L=256 d=40 fused bf16"] = run(A.aliased_attention_tape(BF, DEV, 256, 2, 40), 80, 256, None)
    return out


# ================================================================================================ U-Nets
def _unet(kind):
    from _util import load_golden
    if kind == "sd":
        from oracle import unet_sd
        f = load_golden("decoder_zt_tiny.pt")
        cfg = unet_sd.SDConfig(**f["cfg"])
        return cfg, unet_sd.init_params(cfg, seed=f["seed"], gain=f["gain"]), f["z"], f["ctx"], float(f["t"])
    from oracle import unet_ddpm
    f = load_golden("decoder_xt_ddpm.pt")
    cfg = unet_ddpm.DDPMConfig(**f["cfg"])
    return cfg, unet_ddpm.init_params(cfg, seed=f["seed"]), f["x"], None, float(f["t"])


def _orthonormal(n, cols, seed):
    return torch.linalg.qr(torch.randn(cols, n, generator=torch.Generator().manual_seed(seed)))[0].T.contiguous().to(DEV)


def _unet_group(kind, taps):
    """every entry point on the tiny U-Net: 3x3 / strided / upsampling convolutions, both residual adjoints, concat with both operands active (encoder
    passes) and with an inactive one (passes seeded at a tap: the skip half of every up-block concat), materialised attention, SiLU, the forward-only
    entry points, the power iteration eager and captured"""
    from diffusion_pullback_amd import PullbackUNet
    L, lib = _L()
    cfg, p, x1, c1, t = _unet(kind)
    x = torch.cat([x1, x1.flip(-1)])
    ctx = None if c1 is None else torch.cat([c1, c1.flip(-1)])
    out = {}
    for dtype in (BF, F32):
        dn = NAME[dtype]
        e = PullbackUNet(kind, cfg, p, dtype=dtype, device=DEV, max_batch=B, max_rank=NT, verbose=False).engine
        n_eps = e.tap_numel("eps")
        e.primal(x, t, ctx, "eps")
        r = [_stat(e)]
        e.jvp("eps", _rand(NT, e.n_in, seed=1)); r.append(_stat(e))
        e.vjp("eps", _rand(NT, n_eps, seed=2)); r.append(_stat(e))
        out[f"primal, jvp, vjp eps {dn}"] = r
        if dtype == F32:
            continue
        for tap in taps:
            e.primal(x, t, ctx, "eps")
            r = []
            e.jvp_between(tap, "eps", _rand(NT, e.tap_numel(tap), seed=3)); r.append(_stat(e))
            e.vjp_between(tap, "eps", _rand(NT, n_eps, seed=4)); r.append(_stat(e))
            e.iterate_between(tap, "eps", _orthonormal(NT, e.tap_numel(tap), 5), 2); r.append(_stat(e))
            out[f"jvp_between, vjp_between, iterate_between {tap}->eps {dn}"] = r
        mid = ("mid", 0)
        e.primal(x, t, ctx, mid)
        e.iterate(mid, _orthonormal(NT, e.n_in, 6), 3)
        out[f"iterate mid {dn}"] = [_stat(e)]
        r = []
        e.forward(x, t, ctx, "eps"); r.append(_stat(e))
        e.forward(x[:1], t, None if ctx is None else ctx[:1], mid); r.append(_stat(e))
        e.forward_from(x, t, ctx, mid, _rand(B, e.tap_numel(mid), seed=7)); r.append(_stat(e))
        out[f"forward eps, forward mid, forward_from mid {dn}"] = r
        for tap in taps:
            u = _rand(2, e.tap_numel(tap), seed=8)
            r = []
            e.forward_shift(x[:1], t, None if ctx is None else ctx[:1], tap, u, [-1, 1], [0.0, 0.5]); r.append(_stat(e))     # shared prefix: xbatch 1
            e.forward_shift(x, t, ctx, tap, u, [0, 1], [0.5, -1.0]); r.append(_stat(e))                                       # xbatch = batch
            out[f"forward_shift xbatch=1, xbatch=batch {tap} {dn}"] = r
        # the power iteration on a non-default stream: eager, captured + replayed, replayed from the cached graph (same buffers: same graph key)
        st = torch.cuda.Stream(DEV)
        r = []
        try:
            with torch.cuda.stream(st):
                e.primal(x, t, ctx, mid)
                V0 = _orthonormal(NT, e.n_in, 9)
                V = V0.clone(); U = torch.empty(NT, e.tap_numel(mid), device=DEV); s = torch.empty(NT, device=DEV); conv = torch.empty(B, 2, device=DEV)
                e._set_stream()
                for mode in (0, 1, 1):
                    L.check(lib.dpb_debug_set(b"graph_iterate", mode))
                    V.copy_(V0)
                    L.check(lib.dpb_pullback_iterate(e.h, e.tape.taps[mid], V.data_ptr(), U.data_ptr(), s.data_ptr(), conv.data_ptr(), K, 4))
                    st.synchronize()
                    r.append(_stat(e))
        finally:
            L.check(lib.dpb_debug_set(b"graph_iterate", 0))
        out[f"iterate mid on a stream: eager, captured, cached graph {dn}"] = r
        del e
    return out


def group_unet_sd():
    return _unet_group("sd", [("mid", 0), ("up", 0), ("up", 1)])


def group_unet_ddpm():
    return _unet_group("ddpm", [("mid", 0), ("up", 2), ("up", 0)])


def group_sd_320():
    """one 320-channel level at 16 x 16 with 77 context rows, bf16: the LayerNorm fused into the C = 320 products (ln_fuse 0 and 1), GEGLU in the
    FF-in / FF-out epilogues (tangent, adjoint, forward only), fused attention at L = 256, the one-launch cross attention"""
    from diffusion_pullback_amd import PullbackUNet
    from oracle import unet_sd
    cfg = unet_sd.SDConfig(block_out_channels=(320,), layers_per_block=1, down_attn=(True,), up_attn=(True,), heads=(8,), cross_dim=64,
                           sample_size=16, ctx_len=77)
    p = unet_sd.init_params(cfg, seed=5)
    x, ctx = _rand(B, 4, 16, 16, seed=1), _rand(B, 77, 64, seed=2)
    tap = ("mid", 0)
    e = PullbackUNet("sd", cfg, p, dtype=BF, device=DEV, max_batch=B, max_rank=NT, upto=tap, verbose=False).engine
    out = {}
    for fuse in (0, 1):
        with _switches(ln_fuse=fuse):
            out[f"primal, jvp, vjp mid ln_fuse={fuse}"] = _three(e, x, ctx, tap, e.tap_numel(tap))
    for gf, cp in ((1, 1), (0, 1), (1, 0)):
        with _switches(geglu_fwd=gf, cross_primal=cp):
            e.forward(x, 696.2727, ctx, tap)
            out[f"forward mid geglu_fwd={gf} cross_primal={cp}"] = [_stat(e)]
    return out


GROUPS = {"norm_ops": group_norm_ops, "split_k": group_split_k, "attention": group_attention, "unet_sd": group_unet_sd, "unet_ddpm": group_unet_ddpm,
          "sd_320": group_sd_320}


def record(group):
    """{"<group>/<case>": [[launches, flops, gbytes] per pass]} of one group, from the library lib.load() finds (DPB_LIB or the tree's)"""
    env = sorted(k for k in os.environ if k.startswith("DPB_") and k != "DPB_LIB")
    assert not env, f"the counts are those of the default switches: unset {env}"
    return {f"{group}/{k}": v for k, v in GROUPS[group]().items()}


def write(path, commit, stats):
    """one entry per line (floats as repr: they read back exactly)"""
    with open(path, "w") as fh:
        fh.write('{"commit": %s, "batch": %d, "directions": %d, "stats": {\n' % (json.dumps(commit), B, K))
        fh.write(",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(stats.items())))
        fh.write("\n}}\n")


if __name__ == "__main__":
    assert len(sys.argv) == 2, "usage: DPB_LIB=<build of the recorded commit> make_golden_launch_counts.py <commit hash>"
    stats = {}
    for name in GROUPS:
        stats.update(record(name))
    write(OUT, sys.argv[1], stats)
    print(f"{OUT}: {len(stats)} entries, {sum(len(v) for v in stats.values())} passes of commit {sys.argv[1]}, {os.path.getsize(OUT)} bytes")
