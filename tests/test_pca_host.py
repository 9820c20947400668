"""CPU checks of the global h-space PCA (dpb_pca_lowrank, PullbackUNet.global_pca_zt / inv_jac_zt): the Gram-orthonormalisation restatement
against the reference's own torch.pca_lowrank golden, the exported symbols and their limits, and the ISA of the product kernels."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from _pca_ref import golden_R, golden_zt, pca_lowrank_gram
from _util import abs_cos, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _features(g, case):
    from oracle import unet_sd
    cfg = unet_sd.SDConfig(**g["cfg"])
    p = unet_sd.init_params(cfg, seed=g["seed"], gain=g["gain"])
    zt = golden_zt(case)
    with torch.no_grad():
        h = unet_sd.forward(p, cfg, zt, g["t"], g["ctx"].expand(zt.shape[0], -1, -1), stop=(case["op"], case["idx"]))
    return h.reshape(zt.shape[0], -1)


def test_gram_restatement_matches_the_reference_pca_lowrank():
    g = load_golden("pca_zt_tiny.pt")
    assert len(g["pca"]) >= 4 and any(c["n"] >= 1024 for c in g["pca"]) and any(c["n"] % c["memory_bound"] for c in g["pca"])
    for c in g["pca"]:
        H = _features(g, c)
        assert tuple(golden_R(c).shape) == (min(H.shape), c["q"])
        u, s = pca_lowrank_gram(H, golden_R(c), c["q"], c["niter"])
        assert ((s.double() - c["s"].double()).abs() / c["s"].double()).max() <= 1e-5, (c["n"], c["q"])
        cos = abs_cos(u, c["u"].T)
        assert cos.min() >= 0.9999, (c["n"], c["q"], cos.min())


def test_golden_inv_jac_is_the_normalised_negative_vjp():
    """inv_jac_zt's closed form (vT = -J^T u / ||J^T u||) against the reference's autograd-of-a-norm, on the golden's own net"""
    from oracle import unet_sd
    g = load_golden("pca_zt_tiny.pt")
    cfg = unet_sd.SDConfig(**g["cfg"])
    p = unet_sd.init_params(cfg, seed=g["seed"], gain=g["gain"])
    for c in g["inv"]:
        z = g["z"].clone().requires_grad_(True)
        h = unet_sd.forward(p, cfg, z, g["t"], g["ctx"], stop=(c["op"], c["idx"]))
        (w,) = torch.autograd.grad(h, z, c["u"].reshape(h.shape))
        v = -w.reshape(1, -1) / w.norm()
        assert abs_cos(v, c["vT"]).min() >= 0.99999 and (v * c["vT"]).sum() > 0, c["name"]


def _lib():
    path = os.path.join(ROOT, "diffusion_pullback_amd", "libdpb.so")
    if not os.path.exists(path):
        from diffusion_pullback_amd import lib
        lib.build()
    return ctypes.CDLL(path)


def test_pca_symbols_are_exported_and_declared():
    from diffusion_pullback_amd import lib
    for name in ("dpb_pca_scratch_bytes", "dpb_pca_lowrank"):
        assert name in lib.SYMBOLS
        getattr(_lib(), name)
    with open(os.path.join(ROOT, "include", "dpb.h")) as fh:
        hdr = fh.read()
    assert "size_t dpb_pca_scratch_bytes(int q, int64_t N, int64_t D);" in hdr
    assert re.search(r"int dpb_pca_lowrank\(const float\* H, int64_t N, int64_t D, const float\* R, int q, int niter", hdr)


def test_pca_scratch_bytes_limits():
    lib = _lib()
    f = lib.dpb_pca_scratch_bytes
    f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_int, ctypes.c_int64, ctypes.c_int64]
    assert f(8, 40, 1024) > 0 and f(128, 1000, 81920) > 0 and f(39, 40, 1024) > 0 and f(8, 2000, 8) > 0
    for q, n, d in [(0, 40, 1024), (129, 1000, 81920), (40, 40, 1024), (41, 40, 1024), (8, 40, 0), (9, 2000, 8), (1, 1, 10)]:
        assert f(q, n, d) == 0, (q, n, d)
    # past 4 GiB of H (the up3 tap at N = 900): the size is a 64-bit count that covers the q x D work buffers
    assert f(4, 900, 1310720) > 2 * 4 * 1310720 * 4


def test_pca_lowrank_error_message_without_gpu_work():
    """an invalid shape fails through dpb_last_error before anything touches the device"""
    lib = _lib()
    lib.dpb_last_error.restype = ctypes.c_char_p
    fn = lib.dpb_pca_lowrank
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    dummy = ctypes.c_void_p(16)
    assert fn(dummy, 40, 1024, dummy, 129, 5, dummy, dummy, None, 0, None) != 0
    assert b"q outside [1, 128]" in lib.dpb_last_error()
    assert fn(dummy, 40, 1024, dummy, 40, 5, dummy, dummy, None, 0, None) != 0
    assert b"N - 1" in lib.dpb_last_error()
    assert fn(dummy, 40, 1024, dummy, 8, 5, dummy, dummy, None, 0, None) != 0
    assert b"scratch" in lib.dpb_last_error()


def test_pca_product_kernels_use_fp32_mfma_and_do_not_spill(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this machine")
    out = tmp_path / "pca.s"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-unused-command-line-argument",
                        os.path.join(ROOT, "diffusion_pullback_amd", "csrc", "pca.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    names = re.findall(r"^(_ZN3dpb2[34]pca_prod_(?:samples|features)_kernelILi[1-4]EEEv\w*):", text, flags=re.M)
    assert len(names) == 8, names
    for name in names:
        body = text.split(name + ":", 1)[1].split(".Lfunc_end")[0]
        assert re.search(r"v_mfma_f32_(32x32x2|16x16x4)_f32", body), name
        assert not re.search(r"v_mfma_f32_\w+_(bf16|f16|xf32)", body), name
        assert "scratch_" not in body and "buffer_store" not in body, name
    for meta in re.findall(r"\.name:\s+(_ZN3dpb2[34]pca_prod\w+)\s*\n(.*?)(?=\n\s+- |\n\.end_amdgpu_metadata)", text, flags=re.S):
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta[1]), meta[0]
        assert re.search(r"\.vgpr_spill_count:\s+0\b", meta[1]), meta[0]
