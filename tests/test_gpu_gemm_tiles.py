"""Every forced GEMM tile code (dpb_debug_set("gemm_tile"), include/dpb.h) launches the kernel family it names and computes what the BK = 64 ring
(code 515) computes.  With profiling on, each launch is bracketed with the profile kind of the tile the dispatch planned: the `big` column of
dpb_engine_profile_dump must be the kind include/dpb.h documents for the forced code -- the label bench.py's roofline sorts launches by -- and
primal, tangent and cotangent must equal the code-515 run bit for bit (same K16 MFMA sequence per output element; the halo-tile convolution
accumulates chunk-major: 2e-3 relative, as in test_gpu_parity.py).  Code 515 itself, like every other forced code, is pinned to an fp64 reference in
tests/test_gpu_product_ops.py."""
import csv

import pytest
import torch

pytestmark = pytest.mark.gpu

# forced code -> profile kind of (primal, tangent, cotangent) on a 16 x 16, 320 -> 320 channel 1x1 convolution: M = 256, N = K = 320
KIND_16BIT = {64: 0, 129: 2, 131: 2, 133: 2, 257: 2, 65: 3, 67: 3, 512: 4, 513: 4, 514: 4, 515: 4, 516: 4, 517: 4, 521: 4, 522: 4, 523: 4, 518: 6, 530: 11,
              540: 12}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _engine(H, cin, cout, ks, dtype, g):
    from diffusion_pullback_amd import lib as L
    from diffusion_pullback_amd.engine import Engine
    from diffusion_pullback_amd.tape import Tape
    p = {"c.weight": torch.randn(cout, cin, ks, ks, generator=g) * 0.05, "c.bias": torch.randn(cout, generator=g)}
    t = Tape(p, dtype, _dev())
    t.temb_in = t.buf(1, 8, L.BUF_SHARED)
    t.x = t.buf(H * H, cin)
    o = t.conv("c", t.x, (H, H), cout, ks=ks, stride=1, pad=ks // 2)
    t.tap("o", o, cout, H, H)
    e = Engine(t, 8, False, True, cin, max_batch=1, max_tangents=1)
    x = torch.randn(1, cin, H, H, generator=g).cuda()
    V = torch.randn(1, cin * H * H, generator=g).cuda()
    U = torch.randn(1, cout * H * H, generator=g).cuda()
    return e, x, V, U


def _forced_run(lib, L, e, x, V, U, code, path):
    """one primal + jvp + vjp under the forced code, profiling on -> (outputs, the `big` column of the dump)"""
    L.check(lib.dpb_debug_set(b"gemm_tile", code))
    e.profile(True)
    e.primal(x, 1.0, None, "o")
    outs = (e.read("o").clone(), e.jvp("o", V).clone(), e.vjp("o", U).clone())
    e.profile_dump(str(path))
    e.profile(False)
    with open(path) as fh:
        kinds = [int(r["big"]) for r in csv.DictReader(fh)]
    assert all(torch.isfinite(o).all() for o in outs), code
    return outs, kinds


def test_forced_tile_codes_are_bracketed_with_their_documented_kind_and_match_the_515_run(tmp_path):
    from diffusion_pullback_amd import lib as L
    lib = L.load()
    g = torch.Generator().manual_seed(11)
    try:
        e, x, V, U = _engine(16, 320, 320, 1, torch.bfloat16, g)
        ref, kinds = _forced_run(lib, L, e, x, V, U, 515, tmp_path / "p.csv")
        assert kinds == [4, 4, 4], kinds
        for code, kind in KIND_16BIT.items():
            got, kinds = _forced_run(lib, L, e, x, V, U, code, tmp_path / "p.csv")
            # the primal product carries a bias, which the weights-resident kernel does not take: the documented substitute 515 (kind 4) runs it
            assert kinds == ([4, kind, kind] if code == 540 else [kind] * 3), (code, kinds)
            for a, b, name in zip(ref, got, ("primal", "jvp", "vjp")):
                assert torch.equal(a, b), f"code {code} {name}: max |d| = {(a - b).abs().max().item():.3e}"
        del e
        e, x, V, U = _engine(16, 320, 320, 1, torch.float32, g)       # the register-staged 128x128 tile is the fp32 engine's
        ref, kinds = _forced_run(lib, L, e, x, V, U, 515, tmp_path / "p.csv")
        assert kinds == [0, 0, 0], kinds                              # fp32 never leaves the register-staged kernel: the heuristic's 64x64 tile
        got, kinds = _forced_run(lib, L, e, x, V, U, 128, tmp_path / "p.csv")
        assert kinds == [1, 1, 1], kinds
        for a, b, name in zip(ref, got, ("primal", "jvp", "vjp")):
            assert torch.equal(a, b), f"code 128 (fp32) {name}: max |d| = {(a - b).abs().max().item():.3e}"
        del e
        e, x, V, U = _engine(16, 64, 128, 3, torch.bfloat16, g)       # 3x3 convolution: the halo-tile kernel (forward and adjoint gather)
        ref, kinds = _forced_run(lib, L, e, x, V, U, 515, tmp_path / "p.csv")
        assert kinds == [4, 4, 4], kinds
        got, kinds = _forced_run(lib, L, e, x, V, U, 600, tmp_path / "p.csv")
        assert kinds == [5, 5, 5], kinds
        for a, b, name in zip(ref, got, ("primal", "jvp", "vjp")):
            assert (a - b).norm() <= 2e-3 * a.norm(), f"code 600 {name}: rel {((a - b).norm() / a.norm()).item():.3e}"
    finally:
        L.check(lib.dpb_debug_set(b"gemm_tile", 0))
