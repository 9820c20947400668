"""Not a test: times the Grassmann geodesic (dpb_grassmann_pair, mode 2) at the sizes of the saved local bases: D = 8 pairs of k = 50 rows, T = 9 points.
    python tools/gpu_grassmann_bench.py [--n 16384,32768,81920,196608] [--d 8] [--k 50] [--t 9] [--reps 5] [--out FILE.jsonl]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/gpu_grassmann_bench.py --leg trace --n-one 196608
    python tools/gpu_grassmann_bench.py --leg split --stats DIR/.../t_kernel_stats.csv --n-one 196608 --calls 3 [--out FILE.jsonl]
N: 16 384 (SD x), 32 768 (DDPM h), 81 920 (SD h), 196 608 (DDPM x).  The set: Gaussian rows; per pair 10 rows shared by both bases, the other 40 rows
of B those of A plus Gaussian noise of the same size, so ten angles are zero and the rest lie around pi/4.  Every size runs in a fresh child process under
its own time limit (--leg-timeout seconds); the first that fails or runs out of time ends the run.  One JSON line per size, appended to --out as well; every time is the median of --reps after a warm-up,
device-synchronised:
  geodesic_ms            geometry.grassmann_geodesic(A, B, ts, check=False): the Grams, the whitening, the pair kernel and the stream
  out_gbytes             the bytes of Y [D, T, k, N] fp32, and geodesic_out_gbytes_per_s: those bytes over the whole call
  copy_ms                a device-to-device copy of as many bytes as Y holds, in the same run; copy_write_gbytes_per_s: bytes written over its time
  log_ms, exp_ms         grassmann_log, and grassmann_exp on its (P, H) at the same ts
  torch_fp64_ms          the float64 torch composition of tests/_grassmann_ref.py on the same GPU (batched qr, inverse, thin svd, the T points)
  angle_vs_torch         the largest principal angle between a point here and the composition's, over every t of the first and the last pair (float64)
  exp_log_angle          the largest principal angle between grassmann_exp(grassmann_log(A, B)) and grassmann_geodesic(A, B) over the same points
The split of a call into its kernels comes from a rocprofv3 run of its own (legs `trace` and `split`): the cross-Gram launches, the per-pair algebra,
the stream with its write bandwidth, the rest."""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


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


def _set(d, k, n, shared=10, seed=97):
    import torch
    g = torch.Generator(device=DEV).manual_seed(seed)
    a = torch.randn(d, k, n, generator=g, device=DEV)
    b = a + torch.randn(d, k, n, generator=g, device=DEV)          # every own direction about pi/4 from its partner: well inside the log map's domain
    s = min(shared, k)
    b[:, :s] = a[:, :s]
    return a, b


def _times(t):
    return [-0.5 + 2.0 * j / max(t - 1, 1) for j in range(t)]      # -0.5 .. 1.5: both ends extrapolated


def _torch_geodesic(a, b, ts):
    """tests/_grassmann_ref.py in float64 torch, batched over the pairs: [D, T, N, k] orthonormal columns"""
    import torch
    y0 = torch.linalg.qr(a.double().transpose(1, 2)).Q
    y1 = torch.linalg.qr(b.double().transpose(1, 2)).Q
    m = y0.transpose(1, 2) @ y1
    delta = (y1 - y0 @ m) @ torch.linalg.inv(m)
    u, s, vt = torch.linalg.svd(delta, full_matrices=False)
    th = torch.atan(s)
    y0v = y0 @ vt.transpose(1, 2)
    out = [(y0v * torch.cos(t * th)[:, None, :] + u * torch.sin(t * th)[:, None, :]) @ vt for t in ts]
    return torch.stack(out, dim=1)


def _angle(y_rows, ref_cols):
    """largest principal angle between the row span of y_rows [k, N] (fp32) and the column span of ref_cols [N, k] (orthonormal, fp64): the sine side"""
    import torch
    q = torch.linalg.qr(y_rows.double().T).Q
    gap = q - ref_cols @ (ref_cols.T @ q)
    return float(torch.asin(torch.linalg.svdvals(gap).max().clamp(max=1.0)))


def _size_leg(a):
    import torch
    from diffusion_pullback_amd import geometry as G
    d, k, n, ts = a.d, a.k, a.n_one, _times(a.t)
    out_bytes = 4.0 * d * len(ts) * k * n
    rec = dict(leg="size", D=d, k=k, T=len(ts), N=n, seed=a.seed, in_gbytes=round(8.0 * d * k * n / 1e9, 3), out_gbytes=round(out_bytes / 1e9, 3))
    A, B = _set(d, k, n, seed=a.seed)
    dt, runs = _timed(lambda: G.grassmann_geodesic(A, B, ts, check=False), a.reps)
    rec.update(geodesic_ms=round(dt * 1e3, 3), geodesic_ms_runs=runs, geodesic_out_gbytes_per_s=round(out_bytes / dt / 1e9, 1))
    src = torch.empty(d * len(ts) * k * n, dtype=torch.float32, device=DEV)
    dst = torch.empty_like(src)
    dt, runs = _timed(lambda: dst.copy_(src), a.reps)
    rec.update(copy_ms=round(dt * 1e3, 3), copy_ms_runs=runs, copy_write_gbytes_per_s=round(out_bytes / dt / 1e9, 1))
    del src, dst
    dt, runs = _timed(lambda: G.grassmann_log(A, B, check=False), a.reps)
    rec.update(log_ms=round(dt * 1e3, 3), log_ms_runs=runs)
    P, H, theta = G.grassmann_log(A, B, check=False)
    dt, runs = _timed(lambda: G.grassmann_exp(P, H, ts, check=False), a.reps)
    rec.update(exp_ms=round(dt * 1e3, 3), exp_ms_runs=runs, theta_max=float(theta.max()), theta_min=float(theta.min()))
    Y, _ = G.grassmann_geodesic(A, B, ts, check=False)
    Ye, _ = G.grassmann_exp(P, H, ts, check=False)
    dt, runs = _timed(lambda: _torch_geodesic(A, B, ts), a.reps)
    rec.update(torch_fp64_ms=round(dt * 1e3, 3), torch_fp64_ms_runs=runs)
    ref = _torch_geodesic(A, B, ts)
    pts = [(i, j) for i in sorted({0, d - 1}) for j in range(len(ts))]
    rec["angle_vs_torch"] = max(_angle(Y[i, j], ref[i, j]) for i, j in pts)
    rec["exp_log_angle"] = max(_angle(Ye[i, j], torch.linalg.qr(Y[i, j].double().T).Q) for i, j in pts)
    print(json.dumps(rec), flush=True)


def _trace_leg(a):
    """the work a kernel trace is taken of: --calls geodesic calls"""
    import torch
    from diffusion_pullback_amd import geometry as G
    A, B = _set(a.d, a.k, a.n_one, seed=a.seed)
    for _ in range(a.calls):
        G.grassmann_geodesic(A, B, _times(a.t), check=False)
    torch.cuda.synchronize()


def _split_leg(a):
    rows = list(csv.DictReader(open(a.stats)))
    fam = dict(cross_gram=0.0, pair=0.0, stream=0.0, rest=0.0, other=0.0)
    calls = {}
    for r in rows:
        name, ns, c = r["Name"], float(r["TotalDurationNs"]), int(r["Calls"])
        key = ("cross_gram" if "cross_gram_kernel" in name else "pair" if "gd_pair_kernel" in name else "stream" if "gd_stream_kernel" in name else
               "rest" if ("gram_blocks_kernel" in name or "angles_prep_kernel" in name) else "other")
        fam[key] += ns
        calls[key] = calls.get(key, 0) + c
    per = lambda key: round(fam[key] / 1e6 / a.calls, 4)
    out_bytes = 4.0 * a.d * a.t * a.k * a.n_one
    stream_s = fam["stream"] / 1e9 / a.calls
    rec = dict(leg="split", D=a.d, k=a.k, T=a.t, N=a.n_one, calls=a.calls, source="rocprofv3 --kernel-trace --stats",
               cross_gram_ms=per("cross_gram"), cross_gram_launches=calls.get("cross_gram", 0) // a.calls, pair_ms=per("pair"), stream_ms=per("stream"),
               rest_ms=per("rest"), stream_write_gbytes_per_s=round(out_bytes / max(stream_s, 1e-12) / 1e9, 1),
               stream_mfma_tflops=round(4.0 * a.d * 64 * a.k * a.n_one / max(stream_s, 1e-12) / 1e12, 2))
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="16384,32768,81920,196608")
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--t", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--seed", type=int, default=97)
    ap.add_argument("--leg-timeout", type=int, default=120)
    ap.add_argument("--out", default="")
    ap.add_argument("--stats", default="")
    ap.add_argument("--leg", default="", help=argparse.SUPPRESS)
    ap.add_argument("--n-one", type=int, default=16384, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return {"size": _size_leg, "trace": _trace_leg, "split": _split_leg}[a.leg](a)
    for n in a.n.split(","):
        cmd = ["timeout", "-k", "10", str(a.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", "size", "--n-one", n, "--d", str(a.d),
               "--k", str(a.k), "--t", str(a.t), "--reps", str(a.reps), "--seed", str(a.seed)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:                     # a fault, an abort or a time limit: nothing more is started on the GPU
            print(json.dumps(dict(leg="size", N=int(n), failed=True, returncode=r.returncode, stderr=r.stderr[-800:])), flush=True)
            sys.exit(1)
        print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(lines[-1] + "\n")


if __name__ == "__main__":
    main()
