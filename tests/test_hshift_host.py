"""CPU-only checks of the h-space shifted forward (dpb_forward_shift; PullbackUNet.__call__(u=, op=, block_idx=) / forward_dh / h_traversal):
  * the entry point is in include/dpb.h, in lib.SYMBOLS and in the built library, with 14 arguments; the ABI version stays 1;
  * the reference's own PullBackDDPM.forward(x, t, u, op, block_idx) (tests/golden/make_golden_hshift.py: hshift_ddpm.pt) is the CPU
    restatement of get_h_to_e at input_h = h + u, at 'mid' and every 'up' tap -- the fixture decides where the 'up' tap lies -- so the
    restatement is a fair yardstick for the taps the reference cannot run ('down');
  * the argument checks of the entry point are host code and refuse every case the header lists."""
import ctypes as C
import os
import re

import pytest
import torch

from _decoder_ref import ddpm_h_to_e
from _util import load_golden, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_in_header_symbols_and_library():
    from diffusion_pullback_amd import lib
    with open(os.path.join(ROOT, "include", "dpb.h")) as fh:
        hdr = fh.read()
    m = re.search(r"int\s+dpb_forward_shift\s*\(([^;]*)\)\s*;", hdr)
    assert m, "dpb_forward_shift is not declared in include/dpb.h"
    assert len(m.group(1).split(",")) == 14
    assert re.search(r"#define\s+DPB_ABI_VERSION\s+1\b", hdr)
    res, args = lib.SYMBOLS["dpb_forward_shift"]
    assert res is C.c_int and len(args) == 14
    l = lib.load()
    fn = l.dpb_forward_shift
    assert fn.argtypes == args and fn.restype == res
    assert l.dpb_abi_version() == 1


def test_reference_forward_with_u_is_the_restatement_at_h_plus_u():
    from oracle import unet_ddpm
    f = load_golden("hshift_ddpm.pt")
    cfg = unet_ddpm.DDPMConfig(**f["cfg"])
    p = unet_ddpm.init_params(cfg, seed=f["seed"])
    assert f["down_runs"] is False                                       # diffusion.py:171: the reference's 'down' branch cannot run
    assert [(c["op"], c["idx"]) for c in f["cases"]] == [("mid", 0), ("up", 2), ("up", 1), ("up", 0)]
    with torch.no_grad():
        for c in f["cases"]:
            tap = (c["op"], c["idx"])
            for x, want in ((f["x"], c["eps"]), (f["xb"], c["eps_b"])):
                for b in range(x.shape[0]):
                    h0 = unet_ddpm.forward(p, cfg, x[b:b + 1], f["t"], stop=tap)
                    e = ddpm_h_to_e(p, cfg, x[b:b + 1], f["t"], h0 + c["u"], *tap)
                    assert rel(e, want[b:b + 1]) < 1e-5, (tap, b, rel(e, want[b:b + 1]))


def test_forward_shift_host_checks_without_gpu():
    from oracle import unet_sd
    from diffusion_pullback_amd import lib
    from diffusion_pullback_amd.tape import build_sd
    l = lib.load()
    f = load_golden("decoder_zt_tiny.pt")
    cfg = unet_sd.SDConfig(**f["cfg"])
    p = unet_sd.init_params(cfg, seed=f["seed"], gain=f["gain"])
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
    net.dtype = lib.DPB_F32; net.max_batch = 3; net.max_tangents = 8; net.n_buffers = nb; net.n_ops = no
    net.buffers, net.ops = bufs, ops
    net.x_buf, net.x_channels, net.temb_buf, net.temb_dim = tape.x, cfg.in_channels, tape.temb_in, cfg.block_out_channels[0]
    net.temb_flip_sin_to_cos, net.temb_half_minus_one, net.ctx_buf = 1, 0, tape.ctx
    h = C.c_void_p()
    assert l.dpb_engine_create(C.byref(net), C.byref(h)) == 0, l.dpb_last_error()
    try:
        mid, down, eps = tape.taps[("mid", 0)], tape.taps[("down", 0)], tape.taps["eps"]
        dummy = C.c_void_p(16)

        def call(xb=1, b=2, src=mid, nu=2, dirs=(0, 1, -1), dst=eps):
            d = (C.c_int32 * 4)(*dirs); s = (C.c_float * 4)(1.0, 1.0, 1.0, 1.0)
            rc = l.dpb_forward_shift(h, dummy, xb, b, 1.0, dummy, src, dummy, nu, d, s, dst, 4, dummy)
            return rc, l.dpb_last_error().decode()
        for kw, text in [(dict(b=0), "batch=0 outside"), (dict(b=4), "batch=4 outside"), (dict(xb=2, b=3), "xbatch=2"), (dict(xb=0), "xbatch=0"),
                         (dict(nu=0), "nu=0"), (dict(dirs=(0, 2, 0)), r"dir[1]=2 outside"), (dict(dirs=(-2, 0, 0)), r"dir[0]=-2 outside"),
                         (dict(src=tape.temb_in), "invalid source buffer"), (dict(src=tape.x), "invalid source buffer"),
                         (dict(src=tape.ctx), "invalid source buffer"), (dict(src=-1), "invalid source buffer"),
                         (dict(dst=mid), "not downstream"), (dict(src=mid, dst=down), "not downstream"), (dict(dst=nb), "invalid dst buffer")]:
            rc, err = call(**kw)
            assert rc != 0 and text in err, (kw, rc, err)
        rc, err = call()                                                   # every argument valid: the pass itself needs the workspace
        assert rc != 0 and "workspace" in err, err
        assert l.dpb_forward_shift(h, dummy, 1, 2, 1.0, dummy, mid, None, 2, (C.c_int32 * 2)(0, 1), (C.c_float * 2)(1, 1), eps, 4, dummy) != 0
        assert b"null" in l.dpb_last_error()
    finally:
        l.dpb_engine_destroy(h)


def test_call_surface_without_gpu():
    """the shim's own argument handling needs no engine: SD __call__ with a shift raises TypeError naming forward_dh"""
    from diffusion_pullback_amd.pullback import PullbackUNet
    net = object.__new__(PullbackUNet)
    net.kind = "sd"
    for kw in (dict(u=torch.zeros(1)), dict(uk=torch.zeros(1)), dict(op="mid", block_idx=0)):
        with pytest.raises(TypeError, match="forward_dh"):
            net(torch.zeros(1, 4, 8, 8), 1.0, None, **kw)
    net.kind = "ddpm"
    with pytest.raises(TypeError, match="SD form"):
        net.forward_dh(torch.zeros(1, 3, 8, 8), 1.0, None, op="mid", block_idx=0, uk=torch.zeros(1))
