"""The halo-tile 3x3 convolution's 8-phase main loop (gemm_halo.hip, the default) against its ring loop (dpb_debug_set("halo_loop", 0)).  Both loops
accumulate every output element in the same order (64-channel chunk, then tap, then K16 substep) and partition split-K over the same chunks, so primal,
tangent (forward gather) and cotangent (adjoint gather) products must agree BIT FOR BIT.  The 8-phase loop orders its LDS buffers by counted vmcnt waits
and barriers only (a misplaced read passes whenever the DMA happens to land first): every case runs three times against the reference, and one
configuration is repeated against its own first run."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


# (H, cin, cout, batch): the headline products (SD-1.5 ResBlocks at 5 tangents: 64^2 / 32^2 / 16^2 levels, their 320 -> 640 / 640 -> 1280 convolutions,
# the conv_in adjoint with N = 8 columns of a 128-column tile) and the edge geometries of test_gpu_parity.py's halo cases (16- / 64-pixel rows,
# 8 x 8 images four per tile with a ragged last tile, N tails)
HEADLINE = [(64, 320, 320, 5), (32, 640, 640, 5), (16, 1280, 1280, 5), (32, 320, 640, 5), (16, 640, 1280, 5), (64, 8, 320, 5)]
EDGES = [(32, 320, 320, 5), (16, 128, 200, 2), (64, 64, 136, 1), (8, 128, 136, 5), (16, 192, 72, 3)]


def _engine(H, cin, cout, dtype, batch, g):
    from diffusion_pullback_amd import lib as L
    from diffusion_pullback_amd.engine import Engine
    from diffusion_pullback_amd.tape import Tape
    p = {"c.weight": torch.randn(cout, cin, 3, 3, generator=g) * 0.05, "c.bias": torch.randn(cout, generator=g)}
    t = Tape(p, dtype, _dev())
    t.temb_in = t.buf(1, 8, L.BUF_SHARED)
    t.x = t.buf(H * H, cin)
    o = t.conv("c", t.x, (H, H), cout, ks=3, stride=1, pad=1)
    t.tap("o", o, cout, H, H)
    return Engine(t, 8, False, True, cin, max_batch=batch, max_tangents=batch)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_halo_p8_loop_bitwise_equals_ring_loop_and_race_screen(dtype):
    from diffusion_pullback_amd import lib as L
    lib = L.load()
    g = torch.Generator().manual_seed(5)
    cases = HEADLINE + EDGES if dtype == torch.bfloat16 else HEADLINE[:3] + [HEADLINE[5]] + EDGES[1:]
    try:
        L.check(lib.dpb_debug_set(b"gemm_tile", 600))                 # every product the halo kernel supports runs on it, in both arms
        for (H, cin, cout, batch) in cases:
            e = _engine(H, cin, cout, dtype, batch, g)
            x = torch.randn(batch, cin, H, H, generator=g).cuda()
            V = torch.randn(batch, cin * H * H, generator=g).cuda()
            U = torch.randn(batch, cout * H * H, generator=g).cuda()

            def run():
                e.primal(x, 1.0, None, "o")
                return e.read("o").clone(), e.jvp("o", V).clone(), e.vjp("o", U).clone()
            nch = max(cin, cout) // 64
            for sk in range(1, max(nch, 1) + 1):                      # split-K over 1 .. Cin / 64 chunks (the plan clamps per product)
                L.check(lib.dpb_debug_set(b"gemm_splitk", sk))
                L.check(lib.dpb_debug_set(b"halo_loop", 0)); ref = run()
                assert all(torch.isfinite(r).all() for r in ref)
                L.check(lib.dpb_debug_set(b"halo_loop", 1))
                for rep in range(3):
                    got = run()
                    for a, b, name in zip(ref, got, ("primal", "jvp", "vjp")):
                        assert torch.equal(a, b), f"{dtype} case {(H, cin, cout, batch)} splitk {sk} {name} rep {rep}: max |d| = {(a - b).abs().max().item():.3e}"
            # the comparison means something only where the halo kernel ran (profile kind 5): the forward gather of a Cin % 64 == 0 input in the
            # primal and tangent passes, the adjoint gather of a Cout % 64 == 0 output -- elsewhere both arms run the same implicit-GEMM kernel
            for name, fn, eligible in (("primal", lambda: e.primal(x, 1.0, None, "o"), cin % 64 == 0), ("jvp", lambda: e.jvp("o", V), cin % 64 == 0),
                                       ("vjp", lambda: e.vjp("o", U), cout % 64 == 0)):
                e.profile(True)
                fn()
                n_halo = e.profile_read(5)[0]
                e.profile(False)
                assert (n_halo >= 1) == eligible, f"{dtype} case {(H, cin, cout, batch)} {name}: {n_halo} halo-kernel launches, eligible {eligible}"
            del e
    finally:
        L.check(lib.dpb_debug_set(b"halo_loop", 1))
        L.check(lib.dpb_debug_set(b"gemm_tile", 0)); L.check(lib.dpb_debug_set(b"gemm_splitk", 0))


def test_halo_p8_loop_is_deterministic_run_to_run():
    from diffusion_pullback_amd import lib as L
    lib = L.load()
    g = torch.Generator().manual_seed(6)
    try:
        L.check(lib.dpb_debug_set(b"gemm_tile", 600)); L.check(lib.dpb_debug_set(b"gemm_splitk", 2)); L.check(lib.dpb_debug_set(b"halo_loop", 1))
        for (H, cin, cout, batch) in [(64, 320, 320, 5), (16, 1280, 1280, 5)]:
            e = _engine(H, cin, cout, torch.bfloat16, batch, g)
            x = torch.randn(batch, cin, H, H, generator=g).cuda()
            U = torch.randn(batch, cout * H * H, generator=g).cuda()
            e.primal(x, 1.0, None, "o")
            first = (e.read("o").clone(), e.vjp("o", U).clone())
            for rep in range(20):
                e.primal(x, 1.0, None, "o")
                assert torch.equal(e.read("o"), first[0]) and torch.equal(e.vjp("o", U), first[1]), f"run {rep} of {(H, cin, cout)} differs from the first: a staging race"
            del e
    finally:
        L.check(lib.dpb_debug_set(b"gemm_tile", 0)); L.check(lib.dpb_debug_set(b"gemm_splitk", 0))
