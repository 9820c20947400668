"""CPU checks of local h-space PCA (dpb_perturb_unit, dpb_local_pca_sample, local_pca_zt / local_pca_xt): the integer restatement of the noise
kernel's generator against Philox4x32-10's published known answers, the fixtures' recorded draw sequence against a replay, the closed form of the
x-directions on the golden's own net, and the new symbols of the built library."""
import ctypes
import os

import torch

from _local_pca_ref import philox4x32_10, philox_normals, reference_pairing, replay, unit_open
from _util import abs_cos, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_philox_restatement_reproduces_the_known_answers():
    """the generator's published known-answer vectors (Random123 kat_vectors, philox4x32 with 10 rounds): ctr / key -> out"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, out in kat:
        assert philox4x32_10(ctr, key) == out, [hex(w) for w in philox4x32_10(ctr, key)]


def test_uniform_mapping_is_exact_in_fp32_and_open():
    """include/dpb.h: u(w) = ((w >> 9) + 0.5) * 2^-23 -- an odd multiple of 2^-24: fp32 holds it exactly, it is never 0 and never 1"""
    for w in (0, 1, 511, 512, 0x7fffffff, 0x80000000, 0xfffffdff, 0xffffffff, 0x12345678):
        u = unit_open(w)
        assert 0.0 < u < 1.0
        assert float(torch.tensor(u, dtype=torch.float32)) == u
        assert float(torch.tensor(float(w >> 9), dtype=torch.float32) + 0.5) * 2.0 ** -23 == u      # the kernel's fp32 expression
    assert unit_open(0) == 2.0 ** -24 and unit_open(0xffffffff) == 1 - 2.0 ** -24


def test_restated_normals_are_standard_normal():
    g = torch.cat([philox_normals(7, i, 4096) for i in range(4)])             # 2^14 values: 5 sigma bounds of mean and variance
    n = g.numel()
    assert g.mean().abs() <= 5 / n ** 0.5 and (g.var() - 1).abs() <= 5 * (2 / n) ** 0.5
    assert not torch.equal(philox_normals(7, 0, 8), philox_normals(7, 1, 8)) and not torch.equal(philox_normals(7, 0, 8), philox_normals(8, 0, 8))
    assert torch.equal(philox_normals(7, 2 ** 40 + 5, 7), philox_normals(7, 2 ** 40 + 5, 8)[:7])   # a ragged n is a prefix


def test_fixture_draw_sequences_replay():
    g = load_golden("local_pca_zt_tiny.pt")
    assert [(c["n"], c["memory_bound"], c["q"]) for c in g["cases"]] == [(40, 5, 1), (40, 8, 8), (40, 5, 32), (1040, 104, 8)]
    for c in g["cases"]:
        assert c["d"] == 1024 and c["niter"] == 2 and ("noise" in c) == (c["n"] < c["d"])
        assert c["cond_s"] <= 1e-5 and c["cond_cos"] <= 1e-5                   # the conditioning the generator enforced
        noise, R = replay(c, tuple(g["z"].shape[1:]), generator=torch.Generator())
        assert tuple(noise.shape) == (c["n"], 4, 8, 8) and tuple(R.shape) == (min(c["n"], c["d"]), c["q"])
        assert tuple(c["u"].shape) == (c["d"], c["q"]) and tuple(c["s"].shape) == (c["q"],) and tuple(c["vT"].shape) == (c["q"], 256)
    gd = load_golden("local_pca_xt_ddpm.pt")
    for c in gd["local"]:
        assert c["n"] < c["d"] and c["q"] == 8 and c["cond_s"] <= 1e-5 and c["cond_cos"] <= 1e-5
        replay(c, tuple(gd["x"].shape[1:]), generator=torch.Generator())
    c = gd["global"][0]
    assert torch.equal(torch.randn(c["n"], c["q"], generator=torch.Generator().manual_seed(c["rng_seed"])), c["R"])


def test_golden_x_directions_are_normalised_negative_vjps():
    """The closed form behind vT (the gradient of ||h + p w - get_h(x)|| at x is -w^T J / ||w||) on the golden's own net, for every row of every
    case.  Which w belongs to row i: utils.local_pca_zt adds `u.view(*original_h.shape)` (utils.py:960) -- the ROW-MAJOR VIEW of u [D, q] as
    [q, D], not its transpose -- so its row i is the direction of w_i = u.flatten()[i D : (i + 1) D], a mix of all columns of u when q > 1 (the DDPM
    sibling's inv_jac_xt rearranges properly, diffusion.py:360).  At q = 1 the two coincide.  The product returns the directions of the columns
    of u; tests/test_gpu_local_pca.py therefore meets the SD fixture's vT through the reference's own pairing."""
    from oracle import unet_sd
    g = load_golden("local_pca_zt_tiny.pt")
    cfg = unet_sd.SDConfig(**g["cfg"])
    p = unet_sd.init_params(cfg, seed=g["seed"], gain=g["gain"])
    for c in g["cases"]:
        z = g["z"].clone().requires_grad_(True)
        h = unet_sd.forward(p, cfg, z, g["t"], g["ctx"], stop=(c["op"], c["idx"]))
        W = reference_pairing(c["u"])
        if c["q"] == 1:
            assert torch.equal(W[0], c["u"][:, 0])
        for i in range(c["q"]):
            (w,) = torch.autograd.grad(h, z, W[i].reshape(h.shape), retain_graph=True)
            v = -w.reshape(1, -1) / w.norm()
            assert abs_cos(v, c["vT"][i:i + 1]).min() >= 0.99999 and (v * c["vT"][i]).sum() > 0, (c["q"], i)


def test_new_symbols_resolve_in_the_built_library():
    from diffusion_pullback_amd import lib
    path = os.path.join(ROOT, "diffusion_pullback_amd", "libdpb.so")
    if not os.path.exists(path):
        lib.build()
    so = ctypes.CDLL(path)
    for name in ("dpb_perturb_unit", "dpb_perturb_scratch_bytes", "dpb_local_pca_sample", "dpb_local_pca_scratch_bytes"):
        assert name in lib.SYMBOLS, name
        assert getattr(so, name) is not None
    f = so.dpb_perturb_scratch_bytes
    f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_int, ctypes.c_int64]
    assert f(1, 1) == 8 and f(5, 4096) == 40 and f(5, 4097) == 80 and f(3, 196608) == 3 * 48 * 8      # one fp64 partial per slice of 4096
    assert f(0, 16) == 0 and f(2, 0) == 0
    header = open(os.path.join(ROOT, "include", "dpb.h")).read()
    for name in ("dpb_perturb_unit", "dpb_local_pca_sample", "((w >> 9) + 0.5) * 2^-23", "D2511F53", "utils.py:916-933", "diffusion.py:396-409"):
        assert name in header, name
    assert so.dpb_abi_version() == 1
