"""Not a test: times dpb_subspace_angles at the sizes of the tangent-space job and compares it with what a notebook would do.
    python tools/gpu_subspace_angles_bench.py [--workloads sd_x,sd_h,ddpm_x] [--bases 100] [--k 50] [--reps 3] [--pairs 32] [--out FILE.jsonl]
Workloads (k = 50 rows per basis, B = 100 bases, self mode: all B (B - 1) / 2 pairs): sd_x N = 16 384 (SD latents), sd_h N = 81 920 (SD mid-block
u), ddpm_x N = 196 608 (DDPM / ADM images).  Every leg of every workload runs in a fresh child process under its own time limit (--leg-timeout
seconds); the first leg that fails or runs out of time ends the run.  One JSON line per leg, appended to --out as well:
  ours        geometry.subspace_angles_and_distance on the whole stack: total_ms (median of --reps, device-synchronised), gram_ms -- the
              cross-Gram kernel alone (geometry.cross_gram over all B k rows, the same launches) -- with its achieved fp64 FLOP/s (the upper
              block triangle: (B k)^2 N flops), and rest_ms = total - gram (the B diagonal-block Grams, the whitening and the pair kernel)
  torch_fp64  the float64 torch composition on the same GPU: batched qr -> one matmul of the Q factors -> batched svdvals -> arccos; its worst
              distance from `ours` on small angles is reported, not held to anything (acos loses them even in fp64); "error" if it does not run
  scipy_cpu   scipy.linalg.subspace_angles pair by pair (LAPACK on the process's 16 CPU threads) over --pairs sampled pairs: seconds per pair, the projected time for all
              pairs, and the worst |theta - scipy| of `ours` on that sub-sample
The bases are related Gaussian frames (a shared frame plus 30 % independent noise; every second basis 1e-4 away from its predecessor), so the pairs
carry angles of every size, small ones included."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = {"sd_x": 16384, "sd_h": 81920, "ddpm_x": 196608}
LEGS = ["ours", "torch_fp64", "scipy_cpu"]


def _bases(B, k, N):
    import torch
    g = torch.Generator(device="cuda:0").manual_seed(1234)
    shared = torch.randn(k, N, generator=g, device="cuda:0")
    A = torch.empty(B, k, N, device="cuda:0")
    for b in range(B):                            # basis by basis: no second copy of the stack
        noise = torch.randn(k, N, generator=g, device="cuda:0")
        A[b] = A[b - 1] + 1e-4 * noise if b % 2 else shared + 0.3 * noise
    return A


def _timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), [round(x * 1e3, 3) for x in ts]


def _leg(a):
    import numpy as np
    import torch

    from diffusion_pullback_amd import geometry
    N, B, k = WORKLOADS[a.workload], a.bases, a.k
    A = _bases(B, k, N)
    rec = dict(leg=a.leg, workload=a.workload, B=B, k=k, N=N, pairs=B * (B - 1) // 2)
    if a.leg == "ours":
        total, all_t = _timed(lambda: geometry.subspace_angles_and_distance(A), a.reps)
        gram, all_g = _timed(lambda: geometry.cross_gram(A.view(B * k, N)), a.reps)
        flops = float(B * k) ** 2 * N                    # 2 flops per multiply-add, half of the (B k)^2 entries computed
        rec.update(total_ms=round(total * 1e3, 3), total_ms_runs=all_t, gram_ms=round(gram * 1e3, 3), gram_ms_runs=all_g,
                   gram_fp64_tflops=round(flops / gram / 1e12, 3), rest_ms=round((total - gram) * 1e3, 3),
                   scratch_bytes=int(geometry.L.load().dpb_subspace_angles_scratch_bytes(B, B, k, N)))
    elif a.leg == "torch_fp64":
        theta = geometry.subspace_angles(A)

        def composed():
            Q = torch.linalg.qr(A.double().transpose(1, 2)).Q                    # [B, N, k]
            M = torch.einsum("ink,jnl->ijkl", Q, Q)                               # [B, B, k, k]
            return torch.arccos(torch.linalg.svdvals(M).clamp(max=1.0)).flip(-1)
        try:
            t, all_t = _timed(composed, max(1, a.reps - 1))
            diff = (composed().float() - theta).abs()
            off = ~torch.eye(B, dtype=torch.bool, device=diff.device)
            rec.update(total_ms=round(t * 1e3, 3), total_ms_runs=all_t, worst_abs_diff_from_ours=float(diff[off].max()))
        except Exception as e:                           # the solver routes of the float64 composition are not guaranteed on every build
            rec.update(error=f"{type(e).__name__}: {e}"[:300])
    else:
        from scipy.linalg import subspace_angles
        theta = geometry.subspace_angles(A).cpu().numpy()
        rng = np.random.default_rng(7)
        pairs = [(2 * p, 2 * p + 1) for p in range(min(a.pairs // 2, B // 2))]      # the neighbours 1e-4 apart: the small angles
        while len(pairs) < a.pairs:
            i, j = sorted(rng.choice(B, size=2, replace=False).tolist())
            pairs.append((i, j))
        need = sorted({i for p in pairs for i in p})
        host = {i: A[i].cpu().numpy().astype(np.float64).T for i in need}
        t0 = time.perf_counter()
        refs = [subspace_angles(host[i], host[j]) for i, j in pairs]       # one pair at a time: LAPACK's own threads (concurrent calls from Python
        dt = time.perf_counter() - t0                                      # threads returned wrong angles at N = 196 608 with the BLAS in use)
        worst = max(float(np.abs(theta[i, j] - r).max()) for (i, j), r in zip(pairs, refs))
        rec.update(sampled_pairs=len(pairs), seconds_sampled=round(dt, 3), seconds_per_pair_16_threads=round(dt / len(pairs), 4),
                   projected_seconds_all_pairs=round(dt / len(pairs) * rec["pairs"], 1), worst_abs_theta_minus_scipy=worst)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="sd_x,sd_h,ddpm_x")
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--bases", type=int, default=100)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--leg-timeout", type=int, default=150)
    ap.add_argument("--out", default="")
    ap.add_argument("--leg", default="", help=argparse.SUPPRESS)
    ap.add_argument("--workload", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return _leg(a)
    for w in a.workloads.split(","):
        if w not in WORKLOADS:
            ap.error(f"unknown workload {w}: {sorted(WORKLOADS)}")
        for leg in a.legs.split(","):
            cmd = ["timeout", "-k", "10", str(a.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", leg, "--workload", w,
                   "--bases", str(a.bases), "--k", str(a.k), "--reps", str(a.reps), "--pairs", str(a.pairs)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode != 0 or not lines:            # a fault, an abort or a time limit: nothing more is started on the GPU
                print(json.dumps(dict(leg=leg, workload=w, failed=True, returncode=r.returncode, stderr=r.stderr[-600:])), flush=True)
                sys.exit(1)
            print(lines[-1], flush=True)
            if a.out:
                with open(a.out, "a") as fh:
                    fh.write(lines[-1] + "\n")


if __name__ == "__main__":
    main()
