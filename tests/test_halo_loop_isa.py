"""ISA checks of the halo-tile convolution's 8-phase main loop (gemm_halo.hip, halo_p8_loop), on the gfx950 code hipcc emits here (cross-compiles
without a GPU).  The loop orders its LDS fragment reads only by threading the registers through a later `s_waitcnt lgkmcnt(0)` asm, and its LDS-DMA only
by counted vmcnt waits: a compiler that moved a consumer ahead of the wait, spilled, or drained the DMA queue inside the loop would pass the GPU tests
whenever the data happened to land in time."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")


def _regs(s):
    o = set()
    for m in REG.finditer(s):
        if m.group(1) is not None:
            o.add(int(m.group(1)))
        else:
            o.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return o


@pytest.fixture(scope="module")
def halo_isa(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this machine")
    out = tmp_path_factory.mktemp("halo_isa") / "gemm_halo.s"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-unused-command-line-argument",
                        os.path.join(ROOT, "diffusion_pullback_amd", "csrc", "gemm_halo.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    parts = re.split(r"^(_ZN3dpb16conv_halo_kernel\w+):", text, flags=re.M)[1:]
    kernels = {name: body.split(".Lfunc_end")[0] for name, body in zip(parts[0::2], parts[1::2])}
    assert len(kernels) == 8, sorted(kernels)              # {conv, adjoint} x {bf16, f16} x {ring loop, 8-phase loop}
    return text, kernels


def _p8_kernels(kernels):
    p8 = {n: b for n, b in kernels.items() if n.endswith("ELi1EEEvNS_8GemmArgsE")}   # template argument LOOP = 1
    assert len(p8) == 4
    return p8


def test_halo_p8_loop_keeps_fragment_registers_untouched_until_their_wait(halo_isa):
    _, kernels = halo_isa
    n_reads = 0
    for name, body in _p8_kernels(kernels).items():
        lines = body.splitlines()
        last_mfma = max(i for i, ln in enumerate(lines) if "v_mfma_" in ln.split(";")[0])
        pending = set()
        for ln in lines[:last_mfma + 1]:
            ins = ln.split(";")[0].strip()
            if not ins or ins.startswith(".") or ins.endswith(":"):
                continue
            if ins.startswith("s_waitcnt"):
                if "lgkmcnt(0)" in ins:
                    pending.clear()
                continue
            touched = _regs(ins)
            if ins.startswith("ds_read_b128"):
                dst = _regs(ins.split(",")[0])
                assert not (touched - dst) & pending, (name, ins)
                pending |= dst
                n_reads += 1
                continue
            assert not touched & pending, f"{name}: `{ins}` names a fragment register before its s_waitcnt lgkmcnt(0)"
    assert n_reads >= 4 * 9 * 16                            # one unrolled chunk: 9 taps x (8 A + 8 B) fragment reads per kernel


def test_halo_p8_loop_waits_for_dma_by_count_only(halo_isa):
    """Between the first and the last MFMA (the chunk loop) every vmcnt wait is one of the counted waits of the header's phase table -- no drain
    (vmcnt(0)) -- and each of the 18 phases of the unrolled chunk has its own wait."""
    _, kernels = halo_isa
    for name, body in _p8_kernels(kernels).items():
        lines = [ln.split(";")[0].strip() for ln in body.splitlines()]
        mfma = [i for i, ln in enumerate(lines) if ln.startswith("v_mfma_")]
        assert len(mfma) == 9 * 16, (name, len(mfma))      # 9 taps x 2 phases x 8 MFMAs, one chunk unrolled
        loop = lines[mfma[0]:mfma[-1] + 1]
        vm = [int(m) for ln in loop if ln.startswith("s_waitcnt") for m in re.findall(r"vmcnt\((\d+)\)", ln)]
        assert 0 not in vm, f"{name}: vmcnt(0) inside the main loop"
        assert set(vm) <= {3, 4, 5, 6}, (name, sorted(set(vm)))
        assert len(vm) >= 17, (name, vm)                   # the phase-0 wait of the chunk precedes its first MFMA
        assert sum(ln == "s_barrier" for ln in loop) == 2 * 18 - 2, name   # two per phase, minus the one before the first and after the last MFMA


def test_halo_kernels_use_no_scratch(halo_isa):
    text, kernels = halo_isa
    for name, body in kernels.items():
        assert "scratch_" not in body, name
    for m in re.finditer(r"\.private_segment_fixed_size:\s*(\d+)", text):
        assert m.group(1) == "0"
    for m in re.finditer(r"\.vgpr_spill_count:\s*(\d+)", text):
        assert m.group(1) == "0"
