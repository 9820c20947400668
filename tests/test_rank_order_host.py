"""The rank order of the geometry kernels (diffusion_pullback_amd/csrc/rank.h) on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer.

eig_par_kernel (orth.hip) and the pair kernel of angles.hip scatter by rank -- order[rank_desc(lam, k, t)] = t -- and then index LDS and global memory
with what `order` holds.  The scatter is safe only if the ranks are a permutation of 0 .. k-1 for ANY values; under the plain comparison every NaN got
rank 0 and the other slots kept whatever the LDS held.  tests/host/rank_order_host.cpp includes the very header the kernels include and checks, for k in
{1, 2, 5, 6, 16, 17, 33, 64, 65, 97, 128} and value sets with NaN at every kind of position, infinities, signed zeros and ties: a permutation,
descending, NaN first, ties by index.  It is a stand-alone program with the sanitizer runtimes linked statically: no preload, no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [1, 2, 5, 6, 16, 17, 33, 64, 65, 97, 128]
SETS_PER_K = 11                  # check() calls of the program per k (one of them only for k > 2)


def test_rank_order_is_a_permutation_under_asan_ubsan(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this machine")
    clang = next((p for p in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++") if os.path.exists(p)), None)
    assert clang, "hipcc is here but its clang++ is not"
    exe = str(tmp_path / "rank_order_host")
    r = subprocess.run([clang, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libsan", "-I", os.path.join(ROOT, "diffusion_pullback_amd", "csrc"),
                        os.path.join(ROOT, "tests", "host", "rank_order_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    want = sum(SETS_PER_K - (0 if k > 2 else 1) for k in KS)
    assert r.stdout.strip().splitlines()[-1] == f"rank-order ok {want}"
