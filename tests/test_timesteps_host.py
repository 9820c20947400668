"""Host side of the per-sample timestep entry points (dpb_primal_t / dpb_forward_t, include/dpb.h): exported with the documented signatures, and
their argument checks -- all host code -- answer through dpb_last_error.  The one rule for a timestep argument (engine.timesteps).  No GPU."""
import ctypes as C

import pytest
import torch

from _util import load_golden


def _create(l, lib, tape, x_channels, temb_dim, flip, hm1, max_batch=3):
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
    net.dtype = lib.DPB_F32; net.max_batch = max_batch; net.max_tangents = 8; net.n_buffers = nb; net.n_ops = no
    net.buffers, net.ops = bufs, ops
    net.x_buf, net.x_channels, net.temb_buf, net.temb_dim = tape.x, x_channels, tape.temb_in, temb_dim
    net.temb_flip_sin_to_cos, net.temb_half_minus_one, net.ctx_buf = flip, hm1, getattr(tape, "ctx", -1)
    h = C.c_void_p()
    assert l.dpb_engine_create(C.byref(net), C.byref(h)) == 0, l.dpb_last_error()
    return h, (bufs, ops, net)                     # (the descriptors stay alive with the engine)


def _sd_tape(side=8):
    from oracle import unet_sd
    from diffusion_pullback_amd.tape import build_sd
    f = load_golden("pullback_zt_tiny.pt")
    cfg = unet_sd.SDConfig(**{**f["cfg"], "sample_size": side})
    return cfg, build_sd(cfg, unet_sd.init_params(cfg, seed=f["seed"], gain=f["gain"]), torch.float32, "cpu")


def test_library_exports_the_per_sample_entry_points():
    from diffusion_pullback_amd import lib
    l = lib.load()
    for n in ("dpb_primal_t", "dpb_forward_t"):
        assert hasattr(l, n), n
        res, args = lib.SYMBOLS[n]
        assert getattr(l, n).argtypes == args and getattr(l, n).restype == res
    # the scalar entry points with `float t` replaced by `const float* t`
    p, f = lib.SYMBOLS["dpb_primal"][1], lib.SYMBOLS["dpb_primal_t"][1]
    assert len(f) == len(p) == 6 and f[3] == C.POINTER(C.c_float) and p[3] is C.c_float and f[:3] + f[4:] == p[:3] + p[4:]
    p, f = lib.SYMBOLS["dpb_forward"][1], lib.SYMBOLS["dpb_forward_t"][1]
    assert len(f) == len(p) == 8 and f[3] == C.POINTER(C.c_float) and p[3] is C.c_float and f[:3] + f[4:] == p[:3] + p[4:]
    assert l.dpb_abi_version() == 1
    with open(__file__.rsplit("/tests/", 1)[0] + "/include/dpb.h") as fh:
        text = fh.read()
    assert "int dpb_primal_t(dpb_engine* e, const float* x, int batch, const float* t" in text
    assert "int dpb_forward_t(dpb_engine* e, const float* x, int batch, const float* t" in text


def test_invalid_arguments_return_nonzero_with_a_message():
    from diffusion_pullback_amd import lib
    l = lib.load()
    cfg, tape = _sd_tape()
    h, keep = _create(l, lib, tape, cfg.in_channels, cfg.block_out_channels[0], 1, 0, max_batch=3)
    F = C.c_float
    err = lambda: l.dpb_last_error().decode()
    try:
        eps, dummy = tape.taps["eps"], C.c_void_p(16)
        t3 = (F * 3)(696.0, 301.0, 17.5)
        for call in (lambda t, b: l.dpb_primal_t(h, dummy, b, t, dummy, eps), lambda t, b: l.dpb_forward_t(h, dummy, b, t, dummy, eps, 4, dummy)):
            assert call(None, 3) != 0 and "null" in err()
            assert call(t3, 0) != 0 and "outside [1,3]" in err()
            assert call(t3, 4) != 0 and "outside [1,3]" in err()
            assert call((F * 3)(1.0, float("nan"), 2.0), 3) != 0 and "t[1] is not finite" in err()
            assert call((F * 3)(1.0, 2.0, float("inf")), 3) != 0 and "t[2] is not finite" in err()
            # valid timesteps, distinct or equal, pass these checks: the call gets as far as the missing workspace
            assert call(t3, 3) != 0 and "workspace" in err()
            assert call((F * 3)(5.0, 5.0, 5.0), 3) != 0 and "workspace" in err()
        assert l.dpb_primal_t(None, dummy, 1, t3, dummy, eps) != 0 and "null" in err()
    finally:
        l.dpb_engine_destroy(h)


def test_distinct_timesteps_are_refused_on_tapes_without_a_time_embedding():
    """The autoencoder and text-encoder tapes only fill the engine's timestep slot: no op reads it, so samples cannot differ in t"""
    from diffusion_pullback_amd import configs as cf, lib
    from diffusion_pullback_amd.tape import build_vae_decoder
    l = lib.load()
    cfg = cf.VAEConfig(block_out_channels=(32, 64, 64), layers_per_block=1, groups=8, sample_size=32)
    tape = build_vae_decoder(cfg, {k: v for k, v in cf.vae_init_params(cfg).items() if k.startswith(("decoder.", "post_quant_conv"))}, torch.float32, "cpu")
    h, keep = _create(l, lib, tape, cfg.latent_channels, 8, 0, 1, max_batch=2)
    try:
        out, dummy = tape.taps["image"], C.c_void_p(16)
        assert l.dpb_primal_t(h, dummy, 2, (C.c_float * 2)(0.0, 1.0), None, out) != 0
        assert "without a timestep embedding" in l.dpb_last_error().decode()
        assert l.dpb_primal_t(h, dummy, 2, (C.c_float * 2)(1.0, 1.0), None, out) != 0 and "workspace" in l.dpb_last_error().decode()
    finally:
        l.dpb_engine_destroy(h)


def test_a_shared_buffer_read_by_a_per_sample_op_rules_out_distinct_timesteps():
    """Create-time check: only SHARED ops and row biases may read a SHARED buffer.  A tape whose per-sample product reads the timestep slot
    directly still creates and runs at one timestep; distinct ones are refused with the op named."""
    from diffusion_pullback_amd import lib
    l = lib.load()
    A, S = lib.BUF_ACT, lib.BUF_SHARED
    buffers = [(1, 8, S), (16, 8, A), (1, 8, A)]
    bufs = (lib.BufferDesc * 3)(*[lib.BufferDesc(r, c, k, 0) for r, c, k in buffers])
    ops = (lib.OpDesc * 1)()
    w = (C.c_float * 64)()
    o = ops[0]
    o.kind, o.in0, o.in1, o.in2, o.out, o.res, o.rowbias = lib.OP_CONV, 0, -1, -1, 2, -1, -1
    for j, v in enumerate([1, 1, 8, 1, 1, 8, 1, 1, 0, lib.GATHER_NONE, 0, 0]):
        o.ip[j] = v
    o.w[0] = C.addressof(w)
    net = lib.NetDesc()
    net.dtype = lib.DPB_F32; net.max_batch = 2; net.max_tangents = 2; net.n_buffers = 3; net.n_ops = 1
    net.buffers, net.ops = bufs, ops
    net.x_buf, net.x_channels, net.temb_buf, net.temb_dim, net.ctx_buf = 1, 8, 0, 8, -1
    h = C.c_void_p()
    assert l.dpb_engine_create(C.byref(net), C.byref(h)) == 0, l.dpb_last_error()
    try:
        dummy = C.c_void_p(16)
        assert l.dpb_primal_t(h, dummy, 2, (C.c_float * 2)(0.0, 1.0), None, 2) != 0
        assert "op 0 reads SHARED buffer 0 into per-sample buffer 2" in l.dpb_last_error().decode()
        assert l.dpb_primal_t(h, dummy, 2, (C.c_float * 2)(1.0, 1.0), None, 2) != 0 and "workspace" in l.dpb_last_error().decode()
    finally:
        l.dpb_engine_destroy(h)


def _shared_chain_workspace(l, lib, width, max_batch):
    """workspace bytes of a hand-numbered tape: temb [1][width] SHARED -> SiLU -> st [1][width] SHARED, next to a per-sample x [64][512] -> SiLU.
    Only `width` varies between calls: x (131 072 bytes a row set) stays the largest buffer, so the staging areas sized by it do not move."""
    A, S = lib.BUF_ACT, lib.BUF_SHARED
    buffers = [(1, width, S), (1, width, S), (64, 512, A), (64, 512, A)]
    bufs = (lib.BufferDesc * 4)(*[lib.BufferDesc(r, c, k, 0) for r, c, k in buffers])
    ops = (lib.OpDesc * 2)()
    for o, (i, out) in zip(ops, ((0, 1), (2, 3))):
        o.kind, o.in0, o.in1, o.in2, o.out, o.res, o.rowbias = lib.OP_SILU, i, -1, -1, out, -1, -1
    net = lib.NetDesc()
    net.dtype = lib.DPB_F32; net.max_batch = max_batch; net.max_tangents = 4; net.n_buffers = 4; net.n_ops = 2
    net.buffers, net.ops = bufs, ops
    net.x_buf, net.x_channels, net.temb_buf, net.temb_dim, net.ctx_buf = 2, 512, 0, 8, -1
    h = C.c_void_p()
    assert l.dpb_engine_create(C.byref(net), C.byref(h)) == 0, l.dpb_last_error()
    ws = l.dpb_engine_workspace_bytes(h)
    l.dpb_engine_destroy(h)
    return ws


def test_shared_buffers_have_a_row_per_sample_in_the_workspace():
    """Two tapes that differ only in the width of their two SHARED buffers: the workspace grows by max_batch rows of the difference, not by one.
    (With distinct timesteps the SHARED ops of sample b write row b: a one-row buffer would be overrun into its neighbour.)  Both widths are whole
    256-byte units in fp32, so the planner's alignment adds nothing, and exact equality is the bar."""
    from diffusion_pullback_amd import lib
    l = lib.load()
    w0, w1 = 64, 64 + 1024
    for mb in (1, 2, 5):
        grown = _shared_chain_workspace(l, lib, w1, mb) - _shared_chain_workspace(l, lib, w0, mb)
        assert grown == mb * 2 * (w1 - w0) * 4, (mb, grown)


def test_the_timestep_rule():
    from diffusion_pullback_amd.engine import timesteps
    from diffusion_pullback_amd.pullback import _t_shared
    assert timesteps(3, 4) == 3.0 and timesteps(torch.tensor(2.5), 4) == 2.5 and timesteps(torch.tensor([2.5]), 4) == 2.5
    assert timesteps(torch.tensor(696.2727), 1) == float(torch.tensor(696.2727))         # fp32, as the engine takes it
    assert timesteps(torch.tensor([1.0, 2.0, 3.0]), 3) == [1.0, 2.0, 3.0] and timesteps([1, 2], 2) == [1.0, 2.0]
    assert timesteps(torch.tensor([7, 7, 7]), 3) == 7.0 and isinstance(timesteps([7.0, 7.0], 2), float)     # equal: shared
    for bad, b in ((torch.tensor([1.0, 2.0]), 3), (torch.tensor([1.0, 1.0]), 3), ([1.0, 2.0, 3.0], 1), (torch.zeros(0), 2)):
        with pytest.raises(ValueError, match="elements for a batch"):
            timesteps(bad, b)
    assert _t_shared(torch.tensor([4.0, 4.0]), 2, "x") == 4.0 and _t_shared(4, 2, "x") == 4.0
    with pytest.raises(ValueError, match="forward_dh takes one timestep"):
        _t_shared(torch.tensor([4.0, 5.0]), 2, "forward_dh")
    with pytest.raises(ValueError, match="local_pca takes one timestep"):
        _t_shared(torch.tensor([4.0, 5.0, 6.0]), 1, "local_pca")


def test_cli_parses_the_tangent_space_flags():
    """the flags of the reference's tangent-space job (src/main.py:45-91) are flags here, not 'unknown and ignored'; --h_t_list defaults to --h_t"""
    from diffusion_pullback_amd import main as m
    a = m.parse_args(["--note", "t", "--run_sample_encoder_local_tangent_space_zt", "True", "--num_local_basis", "3", "--h_t_list", "0.8, 0.5,0.2",
                      "--fix_t", "True", "--pca_rank", "50"])
    assert a.run_sample_encoder_local_tangent_space_zt is True and a.num_local_basis == 3 and a.h_t_values == [0.8, 0.5, 0.2]
    assert a.fix_t is True and a.fix_xt is False
    a.memory_bound = 5
    assert m.tangent_space_group(a) == 2                 # 9 pairs, 100 tangents at rank 50
    a.pca_rank = 10
    assert m.tangent_space_group(a) == 5                 # ... bounded by memory_bound
    d = m.parse_args(["--note", "t", "--h_t", "0.6"])
    assert d.h_t_values == [0.6] and d.run_sample_encoder_local_tangent_space_zt is False and d.num_local_basis == 10
    with pytest.raises(SystemExit):
        m.parse_args(["--note", "t", "--fix_xt", "True", "--fix_t", "True"])
    with pytest.raises(SystemExit):
        m.parse_args(["--note", "t", "--h_t_list", "0.8;0.5"])
