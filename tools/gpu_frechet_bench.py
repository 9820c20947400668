"""Not a test: times the Grassmann Frechet mean (dpb_frechet_init / _iterate / _finish) at the sizes of the global-basis job, B = 100 local bases of k = 50 rows.
    python tools/gpu_frechet_bench.py [--n 16384,81920,32768,196608] [--b 100] [--k 50] [--reps 5] [--numpy-n 16384,32768] [--out FILE.jsonl]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/gpu_frechet_bench.py --leg steps --n-one 16384 --steps 20
    python tools/gpu_frechet_bench.py --leg split --stats DIR/.../t_kernel_stats.csv --steps 20 --n-one 16384 [--out FILE.jsonl]
N: 16 384 (SD x), 81 920 (SD h), 32 768 and 196 608 (DDPM h and x).  The set: per basis 10 directions shared by all and 40 of its own, Gaussian rows.
Every size runs in a fresh child process under its own time limit (--leg-timeout seconds); the first that fails or runs out of time ends the run.  One JSON
line per size, appended to --out as well; every time is the median of --reps after a warm-up, device-synchronised:
  copy_gbytes_per_s   a device-to-device copy of 1 GiB, bytes read plus bytes written over its time: the yardstick of the two passes below
  init_ms             dpb_frechet_init (the cross-Gram pass over X, the whitening)
  iterate_ms          one Karcher step (tol = 0: never converged), from a call of --steps steps
  finish_ms           dpb_frechet_finish, and finish_x_gbytes_per_s: the bytes of X over it
  torch_fp64_*        the float64 torch composition of tests/_frechet_ref.py on the same GPU (batched over the bases; QR once, then per step the SVD log
                      map, the thin-SVD exp map and a QR): its set-up and its time per step
  numpy_step_ms       the numpy restatement itself on the host's threads, one step (sizes of --numpy-n only: it holds the float64 bases in host memory)
  angle_after_50      the largest principal angle between this library's mean and the torch composition's after 50 fixed steps each (float64 SVD);
                      with --numpy-50 1 also the angle of each to the numpy restatement's own 50 steps.  status_done = 2: a member of the seeded set lies
                      within 1e-6 of pi/2 from the start, the run stopped with the domain flag and its step time is that of empty launches (--seed: another set)
The split of a step into its kernels comes from a rocprofv3 run of its own (legs `steps` and `split` above): the two passes over Ghat (with their
GB/s: 8 R^2 bytes each), the B eigen-solves of the log map, and the rest."""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
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


def _set(b, k, n, shared=10, seed=97):
    import torch
    g = torch.Generator(device=DEV).manual_seed(seed)
    common = torch.randn(shared, n, generator=g, device=DEV)
    x = torch.randn(b, k, n, generator=g, device=DEV)
    x[:, :shared] = common
    return x


class _Mean:
    """the three entry points on one scratch block"""

    def __init__(self, x, cap):
        import torch
        from diffusion_pullback_amd import lib as L
        self.L, self.lib, self.x, self.cap = L, L.load(), x, cap
        self.b, self.k, self.n = x.shape
        self.need = int(self.lib.dpb_frechet_scratch_bytes(self.b, self.k, self.n, cap))
        assert self.need > 0
        self.scratch = torch.empty(self.need, dtype=torch.uint8, device=DEV)
        self.st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.Y = torch.empty(self.k, self.n, device=DEV)
        self.weight = torch.empty(self.k, device=DEV)
        self.theta = torch.empty(self.b, self.k, device=DEV)
        self.info = torch.empty(8 + 2 * cap + 1 + self.b, dtype=torch.float64, device=DEV)

    def init(self):
        self.L.check(self.lib.dpb_frechet_init(self.x.data_ptr(), self.b, self.k, self.n, 0, self.cap, self.scratch.data_ptr(), self.need, self.st))

    def iterate(self, steps):
        self.L.check(self.lib.dpb_frechet_iterate(steps, 1.0, 0.0, self.b, self.k, self.n, self.cap, self.scratch.data_ptr(), self.need, self.st))

    def finish(self):
        self.L.check(self.lib.dpb_frechet_finish(self.x.data_ptr(), self.Y.data_ptr(), self.weight.data_ptr(), self.theta.data_ptr(), self.info.data_ptr(),
                                                 self.b, self.k, self.n, self.cap, self.scratch.data_ptr(), self.need, self.st))


class _TorchMean:
    """tests/_frechet_ref.py in float64 torch, batched over the bases"""

    def __init__(self, x):
        import torch
        self.t = torch
        self.q = torch.linalg.qr(x.double().transpose(1, 2)).Q.transpose(1, 2).contiguous()        # [B, k, N]
        self.y = self.q[0].clone()

    def step(self):
        t = self.t
        u, c, wt = t.linalg.svd(self.y @ self.q.transpose(1, 2))                                   # [B, k, k]
        d = wt @ self.q - c[:, :, None] * (u.transpose(1, 2) @ self.y)
        s = d.norm(dim=2)
        scale = t.where(s > 0, t.atan2(s, c) / s.clamp_min(1e-300), t.zeros_like(s))
        tan = (u @ (scale[:, :, None] * d)).mean(dim=0)
        p, sig, zt = t.linalg.svd(tan, full_matrices=False)
        yn = p @ (t.cos(sig)[:, None] * (p.T @ self.y)) + p @ (t.sin(sig)[:, None] * zt)
        self.y = t.linalg.qr(yn.T).Q.T.contiguous()


def _size_leg(a):
    import torch
    b, k, n = a.b, a.k, a.n_one
    rec = dict(leg="size", B=b, k=k, N=n, seed=a.seed, R=b * k, x_gbytes=round(4.0 * b * k * n / 1e9, 3), ghat_gbytes=round(8.0 * (b * k) ** 2 / 1e9, 3))
    src = torch.empty(1 << 28, dtype=torch.float32, device=DEV)
    dst = torch.empty_like(src)
    dt, _ = _timed(lambda: dst.copy_(src), a.reps)
    rec["copy_gbytes_per_s"] = round(2.0 * src.numel() * 4 / dt / 1e9, 1)
    del src, dst
    x = _set(b, k, n, seed=a.seed)
    m = _Mean(x, max(64, a.steps * (a.reps + 2)))
    dt, runs = _timed(m.init, a.reps)
    rec.update(init_ms=round(dt * 1e3, 3), init_ms_runs=runs, init_x_gbytes_per_s=round(4.0 * b * k * n / dt / 1e9, 1))
    m.init()
    dt, runs = _timed(lambda: m.iterate(a.steps), a.reps)
    rec.update(iterate_ms=round(dt * 1e3 / a.steps, 3), iterate_ms_runs=[round(r / a.steps, 3) for r in runs], steps_per_call=a.steps)
    dt, runs = _timed(m.finish, a.reps)
    rec.update(finish_ms=round(dt * 1e3, 3), finish_ms_runs=runs, finish_x_gbytes_per_s=round(4.0 * b * k * n / dt / 1e9, 1))
    t0 = time.perf_counter()
    ref = _TorchMean(x)
    torch.cuda.synchronize()
    rec["torch_fp64_setup_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    dt, runs = _timed(ref.step, a.reps)
    rec.update(torch_fp64_step_ms=round(dt * 1e3, 3), torch_fp64_step_ms_runs=runs)
    # 50 fixed steps each, from the same start
    ref.y = ref.q[0].clone()
    for _ in range(50):
        ref.step()
    m.init(); m.iterate(50); m.finish()
    ours = torch.linalg.qr(m.Y.double().T).Q
    cosines = torch.linalg.svdvals(ref.y @ ours)
    gap = ours - ref.y.T @ (ref.y @ ours)                     # the sine side: the part of our span outside the reference's
    rec["angle_after_50"] = float(torch.asin(torch.linalg.svdvals(gap).max().clamp(max=1.0)))
    rec["smallest_cosine_after_50"] = float(cosines.min())
    info = m.info.cpu().numpy()
    rec.update(status_done=int(info[2]), cost_start=float(info[8]), cost_after_50=float(info[8 + 50]), grad_norm_start=float(info[8 + m.cap + 1]), grad_norm_after_50=float(info[8 + m.cap + 1 + 49]))
    if str(n) in a.numpy_n.split(","):
        import numpy as np
        import _frechet_ref as R
        xs = x.cpu().numpy()
        qs = [R.orthonormal_rows(v) for v in xs]
        y = qs[0].copy()

        def np_step():
            logs = [R.log_map(y, q)[0] for q in qs]
            return R.exp_map(y, np.mean(logs, axis=0))
        np_step()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter(); np_step(); ts.append(time.perf_counter() - t0)
        rec.update(numpy_step_ms=round(statistics.median(ts) * 1e3, 1), numpy_threads=os.environ.get("OMP_NUM_THREADS", ""))
        if a.numpy_50:                                        # which of the two GPU results the 50-step angle is owed to: both against numpy's own 50 steps
            for _ in range(50):
                y = np_step()
            yn = torch.from_numpy(y).to(DEV)
            side = lambda basis: float(torch.asin(torch.linalg.svdvals(basis - yn.T @ (yn @ basis)).max().clamp(max=1.0)))
            rec.update(angle_after_50_ours_vs_numpy=side(ours), angle_after_50_torch_vs_numpy=side(ref.y.T.contiguous()))
    print(json.dumps(rec), flush=True)


def _steps_leg(a):
    """the work a kernel trace is taken of: init, --steps Karcher steps, finish"""
    import torch
    m = _Mean(_set(a.b, a.k, a.n_one, seed=a.seed), 64 + a.steps)
    m.init(); m.iterate(a.steps); m.finish()
    torch.cuda.synchronize()


def _split_leg(a):
    rows = list(csv.DictReader(open(a.stats)))
    fam = dict(ghat_passes=0.0, log_map_eigensolves=0.0, step_rest=0.0, cross_gram=0.0, init_rest=0.0, finish_stream=0.0, finish_rest=0.0, other=0.0)
    calls = {}
    for r in rows:
        name, ns, c = r["Name"], float(r["TotalDurationNs"]), int(r["Calls"])
        key = ("ghat_passes" if "fr_product_kernel" in name else "log_map_eigensolves" if "fr_basis_kernel" in name else
               "finish_stream" if "fr_stream_kernel" in name else "finish_rest" if "fr_finish" in name else "cross_gram" if "cross_gram_kernel" in name else
               "init_rest" if any(s in name for s in ("gram_blocks_kernel", "fr_whiten", "fr_init_kernel")) else
               "step_rest" if ("fr_" in name or "angles_prep_kernel" in name) else "other")
        fam[key] += ns
        calls[key] = calls.get(key, 0) + c
    R_ = a.b * a.k
    per = lambda key, n: round(fam[key] / 1e6 / n, 4)
    # the product and the log-map kernels run once more in finish; the whitening once more in init (per basis, one launch)
    passes = calls.get("ghat_passes", 0)
    rec = dict(leg="split", B=a.b, k=a.k, N=a.n_one, steps=a.steps, source="rocprofv3 --kernel-trace --stats",
               ghat_pass_ms=round(fam["ghat_passes"] / 1e6 / max(passes, 1), 4), ghat_passes_traced=passes,
               ghat_pass_gbytes_per_s=round(8.0 * R_ * R_ / (fam["ghat_passes"] / max(passes, 1)), 1),
               log_map_eigensolves_ms_per_launch=round(fam["log_map_eigensolves"] / 1e6 / max(calls.get("log_map_eigensolves", 0), 1), 4),
               step_rest_ms_per_step=per("step_rest", a.steps), kernel_ms_per_step=round((fam["ghat_passes"] * 2 * a.steps / max(passes, 1)
               + fam["log_map_eigensolves"] * a.steps / max(calls.get("log_map_eigensolves", 0), 1) + fam["step_rest"]) / 1e6 / a.steps, 4),
               cross_gram_ms=per("cross_gram", 1), init_rest_ms=per("init_rest", 1), finish_stream_ms=per("finish_stream", 1),
               finish_stream_x_gbytes_per_s=round(4.0 * R_ * a.n_one / max(fam["finish_stream"], 1.0), 1), finish_rest_ms=per("finish_rest", 1))
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="16384,81920,32768,196608")
    ap.add_argument("--b", type=int, default=100)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--numpy-n", default="16384,32768")
    ap.add_argument("--seed", type=int, default=97)
    ap.add_argument("--numpy-50", type=int, default=0, help="1: also 50 numpy steps, and the angle of both GPU results to theirs (sizes of --numpy-n)")
    ap.add_argument("--leg-timeout", type=int, default=240)
    ap.add_argument("--out", default="")
    ap.add_argument("--stats", default="")
    ap.add_argument("--leg", default="", help=argparse.SUPPRESS)
    ap.add_argument("--n-one", type=int, default=16384, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return {"size": _size_leg, "steps": _steps_leg, "split": _split_leg}[a.leg](a)
    for n in a.n.split(","):
        cmd = ["timeout", "-k", "10", str(a.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", "size", "--n-one", n, "--b", str(a.b),
               "--k", str(a.k), "--reps", str(a.reps), "--steps", str(a.steps), "--numpy-n", a.numpy_n, "--seed", str(a.seed), "--numpy-50", str(a.numpy_50)]
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
