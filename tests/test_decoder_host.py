"""CPU-only checks of the decoder pullback (J_dec = d eps / d h at a tap, skips held at their primal values):
  * the CPU restatement of get_h_to_e (tests/_decoder_ref.py) plus a plain power loop reproduces every reference golden of
    tests/golden/make_golden_decoder.py (PullBackDDPM.local_decoder_pullback_xt / local_x0_decoder_pullback_xt,
    utils.local_decoder_pullback_zt) -- what the GPU tests compare the engine against is the reference's own result;
  * libdpb.so exports the new entry points with the ctypes signatures of lib.py, and their host-side checks work without a GPU."""
import ctypes as C

import pytest
import torch

from _decoder_ref import ddpm_h_to_e, power_loop, sd_h_to_e
from _util import abs_cos, load_golden

NEW = ("dpb_jvp_between", "dpb_vjp_between", "dpb_pullback_scratch_bytes", "dpb_pullback_iterate_between", "dpb_forward_from")


def _ddpm():
    from oracle import unet_ddpm
    f = load_golden("decoder_xt_ddpm.pt")
    cfg = unet_ddpm.DDPMConfig(**f["cfg"])
    return f, cfg, unet_ddpm.init_params(cfg, seed=f["seed"])


def _sd():
    from oracle import unet_sd
    f = load_golden("decoder_zt_tiny.pt")
    cfg = unet_sd.SDConfig(**f["cfg"])
    return f, cfg, unet_sd.init_params(cfg, seed=f["seed"], gain=f["gain"])


def _check(c, V, s, U, scale=1.0):
    assert c["u"].shape == (V.shape[1], c["k"]) and c["vT"].shape == U.shape
    assert torch.allclose(s * abs(scale), c["s"], rtol=1e-3), (s * abs(scale), c["s"])
    assert (abs_cos(V, c["u"].T) > 0.9999).all(), abs_cos(V, c["u"].T)
    assert (abs_cos(U, c["vT"]) > 0.9999).all(), abs_cos(U, c["vT"])


@pytest.mark.parametrize("case", [0, 1])
def test_restatement_reproduces_ddpm_decoder_golden(case):
    from oracle import unet_ddpm
    f, cfg, p = _ddpm()
    c = f["xt"][case]
    h0 = unet_ddpm.forward(p, cfg, f["x"], f["t"], stop=("mid", 0)).detach()
    V, s, U = power_loop(lambda h: ddpm_h_to_e(p, cfg, f["x"], f["t"], h, "mid", 0), h0, c["V0"], c["iters"])
    _check(c, V, s, U)
    assert c["iters"] == (c["min_iter"] + 2 if c["thr"] >= 0.5 else c["max_iter"])     # one case stops early, one runs to max_iter


@pytest.mark.parametrize("case", [0, 1])
def test_restatement_reproduces_ddpm_x0_decoder_golden(case):
    """x0 = (x - sqrt(1 - a_t) eps) / sqrt(a_t): the reference's own function through the same power loop, and the exact rescale of the
    plain decoder run that PullbackUNet.local_x0_decoder_pullback_xt returns."""
    from oracle import unet_ddpm
    f, cfg, p = _ddpm()
    c = f["x0"][case]
    at = f["at"]
    h0 = unet_ddpm.forward(p, cfg, f["x"], f["t"], stop=("mid", 0)).detach()
    e = lambda h: ddpm_h_to_e(p, cfg, f["x"], f["t"], h, "mid", 0)
    V, s, U = power_loop(lambda h: (f["x"] - (1 - at).sqrt() * e(h)) / at.sqrt(), h0, c["V0"], c["iters"])
    _check(c, V, s, U)
    Vd, sd, Ud = power_loop(e, h0, c["V0"], c["iters"])
    cc = float(-(1 - at).sqrt() / at.sqrt())
    _check(c, Vd, sd, Ud * cc, scale=cc)


@pytest.mark.parametrize("case", [0, 1, 2])
def test_restatement_reproduces_sd_decoder_golden(case):
    from oracle import unet_sd
    f, cfg, p = _sd()
    c = f["cases"][case]
    h0 = unet_sd.forward(p, cfg, f["z"], f["t"], f["ctx"], stop=(c["op"], c["idx"])).detach()
    V, s, U = power_loop(lambda h: sd_h_to_e(p, cfg, f["z"], f["t"], f["ctx"], h, c["op"], c["idx"]), h0, c["V0"], c["iters"])
    _check(c, V, s, U)


def test_restatement_at_primal_tap_is_the_forward():
    """get_h_to_e(h0) with h0 the primal tap value is eps, at every tap of both families"""
    from oracle import unet_ddpm, unet_sd
    f, cfg, p = _sd()
    eps = unet_sd.forward(p, cfg, f["z"], f["t"], f["ctx"])
    for tap in [("down", 0), ("down", 1), ("mid", 0), ("up", 0), ("up", 1)]:
        h0 = unet_sd.forward(p, cfg, f["z"], f["t"], f["ctx"], stop=tap)
        e = sd_h_to_e(p, cfg, f["z"], f["t"], f["ctx"], h0.repeat(2, 1, 1, 1), *tap)
        assert torch.allclose(e, eps.expand(2, -1, -1, -1), atol=1e-5, rtol=1e-4), tap
    f, cfg, p = _ddpm()
    eps = unet_ddpm.forward(p, cfg, f["x"], f["t"])
    for tap in [("down", 0), ("down", 2), ("mid", 0), ("up", 2), ("up", 0)]:
        h0 = unet_ddpm.forward(p, cfg, f["x"], f["t"], stop=tap)
        assert torch.allclose(ddpm_h_to_e(p, cfg, f["x"], f["t"], h0, *tap), eps, atol=1e-5, rtol=1e-4), tap
    with pytest.raises(ValueError):
        ddpm_h_to_e(p, cfg, f["x"], f["t"], h0, "side", 0)


def test_library_exports_decoder_entry_points():
    from diffusion_pullback_amd import lib
    l = lib.load()
    for n in NEW:
        assert hasattr(l, n), n
        res, args = lib.SYMBOLS[n]
        assert getattr(l, n).argtypes == args and getattr(l, n).restype == res
    assert len(lib.SYMBOLS["dpb_jvp_between"][1]) == 6 and len(lib.SYMBOLS["dpb_pullback_iterate_between"][1]) == 11
    assert lib.SYMBOLS["dpb_pullback_scratch_bytes"][0] is C.c_size_t and lib.SYMBOLS["dpb_pullback_iterate_between"][1][-1] is C.c_size_t
    assert len(lib.SYMBOLS["dpb_forward_from"][1]) == 10


def test_decoder_host_checks_without_gpu():
    """engine_create and the argument checks of the new entry points are host code: the scratch size of the decoder iteration grows with
    numel(src) and k, not the engine's workspace; a pass refuses to run without a workspace, a bad source or rank."""
    from oracle import unet_sd
    from diffusion_pullback_amd import lib
    from diffusion_pullback_amd.tape import build_sd
    l = lib.load()
    f, cfg, p = _sd()
    tape = build_sd(cfg, p, torch.float32, "cpu")
    nb, no = len(tape.buffers), len(tape.ops)
    bufs = (lib.BufferDesc * nb)(*[lib.BufferDesc(r, c, k, v) for (r, c, k), v in zip(tape.buffers, tape.valid)])
    ops = (lib.OpDesc * no)()
    for i, d in enumerate(tape.ops):
        o = ops[i]
        o.kind, o.in0, o.in1, o.in2, o.out, o.res, o.rowbias = d["kind"], d["in0"], d["in1"], d["in2"], d["out"], d["res"], d["rowbias"]
        for j in range(12):
            o.ip[j] = int(d["ip"][j])
        for j in range(4):
            o.fp[j] = float(d["fp"][j]); o.w[j] = d["w"][j] or None
    net = lib.NetDesc()
    net.dtype = lib.DPB_F32; net.max_batch = 2; net.max_tangents = 8; net.n_buffers = nb; net.n_ops = no
    net.buffers, net.ops = bufs, ops
    net.x_buf, net.x_channels, net.temb_buf, net.temb_dim = tape.x, cfg.in_channels, tape.temb_in, cfg.block_out_channels[0]
    net.temb_flip_sin_to_cos, net.temb_half_minus_one, net.ctx_buf = 1, 0, tape.ctx
    h = C.c_void_p()
    assert l.dpb_engine_create(C.byref(net), C.byref(h)) == 0, l.dpb_last_error()
    try:
        mid, down = tape.taps[("mid", 0)], tape.taps[("down", 0)]
        eps = tape.taps["eps"]
        n_mid = 64 * 4 * 4
        s3, s6 = l.dpb_pullback_scratch_bytes(h, mid, 3), l.dpb_pullback_scratch_bytes(h, mid, 6)
        assert s3 >= 2 * 3 * n_mid * 4 and s6 > s3                     # W staging of max_batch samples + the orth slots
        assert l.dpb_pullback_scratch_bytes(h, down, 3) > 0
        assert l.dpb_pullback_scratch_bytes(h, mid, 0) == 0 and l.dpb_pullback_scratch_bytes(h, mid, 129) == 0
        assert l.dpb_pullback_scratch_bytes(h, tape.temb_in, 3) == 0                 # a shared (x-independent) buffer is no seed
        dummy = C.c_void_p(16)
        assert l.dpb_jvp_between(h, mid, eps, dummy, 3, dummy) != 0 and b"workspace" in l.dpb_last_error()
        assert l.dpb_forward_from(h, dummy, 1, 1.0, dummy, eps, dummy, mid, 64, dummy) != 0
        assert b"not downstream" in l.dpb_last_error() or b"invalid source" in l.dpb_last_error()
        assert l.dpb_forward_from(h, dummy, 1, 1.0, dummy, mid, dummy, down, 32, dummy) != 0 and b"not downstream" in l.dpb_last_error()
    finally:
        l.dpb_engine_destroy(h)


def _small_net(l, lib, junk=None, concat_in1=2):
    """A hand-numbered tape on x [16][32]: SiLU(temb), GroupNorm, LayerNorm, FF-in product -> GEGLU (interleaved) -> FF-out product (+ x), concat.
    Buffer 0 is the GEGLU input, so any op that wrongly counts as a reader of id 0 trips the "no other consumer" check.  junk: the value written
    into every input id the op kind does not read (in1 / in2 of CONV, GROUPNORM, LAYERNORM, GEGLU, SILU; in2 of CONCAT; res of non-CONV ops);
    None leaves them at -1.  Returns (rc, workspace bytes, error text)."""
    A, S = lib.BUF_ACT, lib.BUF_SHARED
    buffers = [(16, 128, A), (1, 8, S), (16, 32, A), (16, 32, A), (16, 32, A), (16, 64, A), (16, 32, A), (16, 64, A), (1, 8, S)]
    h, temb, x, gn, ln, gg, ff, cat, st = range(9)
    conv = lambda cin, cout: [4, 4, cin, 4, 4, cout, 1, 1, 0, lib.GATHER_NONE, 0, 0]
    # (kind, in0, in1, in2, out, res, ip)
    tape = [(lib.OP_SILU, temb, -1, -1, st, -1, [0] * 12),
            (lib.OP_GROUPNORM, x, -1, -1, gn, -1, [8, 0] + [0] * 10),
            (lib.OP_LAYERNORM, gn, -1, -1, ln, -1, [0] * 12),
            (lib.OP_CONV, ln, -1, -1, h, -1, conv(32, 128)),
            (lib.OP_GEGLU, h, -1, -1, gg, -1, [0, 64] + [0] * 10),
            (lib.OP_CONV, gg, -1, -1, ff, x, conv(64, 32)),
            (lib.OP_CONCAT, ff, concat_in1, -1, cat, -1, [0] * 12)]
    bufs = (lib.BufferDesc * len(buffers))(*[lib.BufferDesc(r, c, k, 0) for r, c, k in buffers])
    ops = (lib.OpDesc * len(tape))()
    weights = (C.c_float * 16)()                   # create only looks at which weight pointers are set
    for o, (kind, in0, in1, in2, out, res, ip) in zip(ops, tape):
        unread_in = kind != lib.OP_CONCAT and junk is not None
        o.kind, o.in0, o.out, o.rowbias = kind, in0, out, -1
        o.in1 = junk if unread_in else in1
        o.in2 = junk if junk is not None else in2
        o.res = junk if junk is not None and kind != lib.OP_CONV else res
        for j in range(12):
            o.ip[j] = ip[j]
        o.fp[0] = 1e-5
        o.w[0] = o.w[1] = C.addressof(weights)
    net = lib.NetDesc()
    net.dtype = lib.DPB_F32; net.max_batch = 2; net.max_tangents = 4; net.n_buffers = len(buffers); net.n_ops = len(tape)
    net.buffers, net.ops = bufs, ops
    net.x_buf, net.x_channels, net.temb_buf, net.temb_dim, net.ctx_buf = x, 32, temb, 8, -1
    e = C.c_void_p()
    rc = l.dpb_engine_create(C.byref(net), C.byref(e))
    err = l.dpb_last_error().decode()
    ws = l.dpb_engine_workspace_bytes(e) if rc == 0 else 0
    if rc == 0:
        l.dpb_engine_destroy(e)
    return rc, ws, err


def test_input_ids_an_op_kind_does_not_read_mean_nothing():
    """include/dpb.h: an input id the op kind does not read means nothing.  The same tape with -1 and with 0 in every such id creates the same
    engine; a genuine second reader of the GEGLU input is still refused."""
    from diffusion_pullback_amd import lib
    l = lib.load()
    rc, ws, err = _small_net(l, lib)
    assert rc == 0 and ws > 0, err
    rc0, ws0, err0 = _small_net(l, lib, junk=0)
    assert rc0 == 0, err0
    assert ws0 == ws
    rc2, _, err2 = _small_net(l, lib, concat_in1=0)                    # CONCAT does read in1: buffer 0 has two consumers
    assert rc2 != 0 and "no other consumer" in err2, err2
