"""Not a test: times the flag mean (dpb_flag_mean_init / _iterate / _finish) on the set of tools/gpu_frechet_bench.py -- B = 100 local bases of k = 50 rows,
10 directions shared by all and 40 of their own, Gaussian rows -- for the ranks r = 10 (inside the gap) and r = 50 (inside the bulk).
    python tools/gpu_flag_mean_bench.py [--n 16384,32768,81920,196608] [--r 10,50] [--reps 5] [--numpy-n 16384] [--karcher-n 16384] [--fm-waves 8|4] [--out FILE.jsonl]
Every size runs in a fresh child process under its own time limit (--leg-timeout seconds); the first that fails or runs out of time ends the run.  One
JSON line per (N, r), appended to --out as well; every time is the median of --reps after a warm-up, device-synchronised, all in one session:
  copy_gbytes_per_s     a device-to-device copy of the bytes of Ghat (8 R^2), bytes read plus written over its time, in the same process
  init_ms               dpb_flag_mean_init (the cross-Gram pass over X, the whitening, the start block)
  iterations, converged, residual, solve_ms   the solve to tol = 1e-12 within --max-iter, status read every 16 iterations
  iterate_ms            one iteration, from a call of --steps iterations with tol = 0
  finish_ms             dpb_flag_mean_finish
  kernels               device time per launch of the kernels of one traced run (torch.profiler): the new product kernel fm_product_kernel with its
                        GB/s of Ghat (to hold against copy_gbytes_per_s: a copy moves twice the bytes it reads), the Frechet mean's fr_product_kernel
                        on the same Ghat (k = 50 columns: four 16-column tiles, as m = 64), the Jacobi heads and the rest of an iteration
  torch_fp64_ms         the float64 torch composition on the same GPU: batched qr, the Gram of the stacked Q's, eigh, the top r rows; angle_to_torch: the
                        largest principal angle between the two results (float64)
  numpy_ms              the same composition in numpy on the host's threads (sizes of --numpy-n), angle_to_numpy
  karcher_steps_*       sizes of --karcher-n, r = k only: Karcher steps to tol 1e-6 within 200 from init = 0 and from init = "flag" """
import argparse
import ctypes as C
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


def _set(b, k, n, shared=10, seed=97):
    import torch
    g = torch.Generator(device=DEV).manual_seed(seed)
    common = torch.randn(shared, n, generator=g, device=DEV)
    x = torch.randn(b, k, n, generator=g, device=DEV)
    x[:, :shared] = common
    return x


class _Flag:
    def __init__(self, x, r, cap):
        import torch
        from diffusion_pullback_amd import lib as L
        self.L, self.lib, self.x, self.r, self.cap = L, L.load(), x, r, cap
        self.b, self.k, self.n = x.shape
        self.need = int(self.lib.dpb_flag_mean_scratch_bytes(self.b, self.k, self.n, r, cap))
        assert self.need > 0
        self.scratch = torch.empty(self.need, dtype=torch.uint8, device=DEV)
        self.st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.Y = torch.empty(r, self.n, device=DEV)
        self.weight = torch.empty(r, device=DEV)
        self.theta = torch.empty(self.b, min(r, self.k), device=DEV)
        self.Ct = torch.empty(self.b * self.k, r, dtype=torch.float64, device=DEV)
        self.info = torch.empty(72 + self.b, dtype=torch.float64, device=DEV)

    def args(self):
        return self.b, self.k, self.n, self.r, self.cap, self.scratch.data_ptr(), self.need, self.st

    def init(self):
        self.L.check(self.lib.dpb_flag_mean_init(self.x.data_ptr(), None, self.b, self.k, self.n, self.r, 0, self.cap, self.scratch.data_ptr(), self.need, self.st))

    def iterate(self, steps, tol):
        self.L.check(self.lib.dpb_flag_mean_iterate(steps, tol, None, *self.args()))

    def solve(self, tol=1e-12, every=16):
        import torch
        self.init()
        asked = 0
        while asked < self.cap:
            steps = min(every, self.cap - asked)
            self.iterate(steps, tol)
            asked += steps
            if int(self.scratch[:4].view(torch.int32).item()) != 0:
                break

    def finish(self):
        self.L.check(self.lib.dpb_flag_mean_finish(self.x.data_ptr(), None, self.Y.data_ptr(), self.weight.data_ptr(), self.theta.data_ptr(),
                                                   self.Ct.data_ptr(), self.info.data_ptr(), *self.args()))


def _angle(torch, ya, yb):
    """largest principal angle between the row spans of ya and yb (float64, the sine side)"""
    qa = torch.linalg.qr(ya.double().T).Q
    qb = torch.linalg.qr(yb.double().T).Q
    return float(torch.asin(torch.linalg.svdvals(qa - qb @ (qb.T @ qa)).max().clamp(max=1.0)))


def _kernel_split(torch, fm, steps, b, k, n):
    """device time per launch by kernel family, from one traced run of `steps` iterations, a finish, two Frechet steps on the same set and a copy"""
    from torch.profiler import ProfilerActivity, profile
    from diffusion_pullback_amd import lib as L
    lib = L.load()
    cap = 8
    need = int(lib.dpb_frechet_scratch_bytes(b, k, n, cap))
    fs = torch.empty(need, dtype=torch.uint8, device=DEV)
    L.check(lib.dpb_frechet_init(fm.x.data_ptr(), b, k, n, 0, cap, fs.data_ptr(), need, fm.st))
    fm.init()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fm.iterate(steps, 0.0)
        fm.finish()
        L.check(lib.dpb_frechet_iterate(2, 1.0, 0.0, b, k, n, cap, fs.data_ptr(), need, fm.st))
        torch.cuda.synchronize()
    fam = {}
    for ev in prof.key_averages():
        name = ev.key
        key = ("fm_product" if "fm_product_kernel" in name else "fr_product" if "fr_product_kernel" in name else
               "fm_heads" if ("fm_head_kernel" in name or "fm_orth_head_kernel" in name) else
               "fm_finish" if any(s in name for s in ("fm_finish", "fm_sign", "fm_coef", "fm_theta", "fr_stream")) else
               "fm_rest" if "fm_" in name else None)
        if key:
            t, c = fam.get(key, (0.0, 0))
            total = getattr(ev, "device_time_total", None)
            total = ev.cuda_time_total if total is None else total
            fam[key] = (t + total, c + ev.count)
    R_ = b * k
    out = {key: dict(us_per_launch=round(t / c, 2), launches=c) for key, (t, c) in fam.items()}
    for key in ("fm_product", "fr_product"):
        if key in out:
            out[key]["ghat_gbytes_per_s"] = round(8.0 * R_ * R_ / (out[key]["us_per_launch"] * 1e-6) / 1e9, 1)
    if "fm_heads" in out and "fm_rest" in out:
        per_iter = lambda key: fam[key][0] / steps
        out["iteration_us"] = dict(product=round(out["fm_product"]["us_per_launch"], 2), heads=round(per_iter("fm_heads"), 2), rest=round(per_iter("fm_rest"), 2))
    return out


def _size_leg(a):
    import numpy as np
    import torch
    b, k, n = a.b, a.k, a.n_one
    R_ = b * k
    x = _set(b, k, n, seed=a.seed)
    src = torch.empty(R_ * R_, dtype=torch.float64, device=DEV)
    dst = torch.empty_like(src)
    dt, _ = _timed(lambda: dst.copy_(src), a.reps)
    copy = round(2.0 * 8 * R_ * R_ / dt / 1e9, 1)
    del src, dst
    t0 = time.perf_counter()
    q = torch.linalg.qr(x.double().transpose(1, 2)).Q.transpose(1, 2).reshape(R_, n)

    def torch_mean(r):
        lam, v = torch.linalg.eigh(q @ q.T)
        return (v[:, -r:].flip(1) / lam[-r:].flip(0).sqrt()).T @ q, lam.flip(0) / b
    torch.cuda.synchronize()
    qr_ms = (time.perf_counter() - t0) * 1e3
    for r in [int(v) for v in a.r.split(",")]:
        rec = dict(leg="size", B=b, k=k, N=n, r=r, R=R_, seed=a.seed, fm_waves=int(os.environ.get("DPB_FM_WAVES", "8")), ghat_gbytes=round(8.0 * R_ * R_ / 1e9, 3), copy_gbytes_per_s=copy)
        fm = _Flag(x, r, a.max_iter)
        dt, runs = _timed(fm.init, a.reps)
        rec.update(init_ms=round(dt * 1e3, 3), init_ms_runs=runs)
        dt, runs = _timed(fm.solve, a.reps)
        fm.finish()
        info = fm.info.cpu().numpy()
        m = int(info[3])
        eig = info[8:8 + m] / b
        rec.update(m=m, iterations=int(info[0]), converged=int(info[1]) == 1, residual=float(info[2]), solve_ms=round(dt * 1e3, 3), solve_ms_runs=runs,
                   spectrum_around_r=[round(float(v), 5) for v in eig[max(0, r - 3):r + 3]], gap=(round(float(eig[r - 1] - eig[r]), 5) if m > r else None))
        y_solved = fm.Y.clone()
        fm.init()
        dt, runs = _timed(lambda: fm.iterate(a.steps, 0.0), a.reps)
        rec.update(iterate_ms=round(dt * 1e3 / a.steps, 4), iterate_ms_runs=[round(v / a.steps, 4) for v in runs], steps_per_call=a.steps)
        dt, runs = _timed(fm.finish, a.reps)
        rec.update(finish_ms=round(dt * 1e3, 3), finish_ms_runs=runs, finish_x_gbytes_per_s=round(4.0 * R_ * n / dt / 1e9, 1))
        try:
            rec["kernels"] = _kernel_split(torch, fm, a.steps, b, k, n)
        except Exception as e:                                 # the profiler is a convenience: the times above stand without it
            rec["kernels"] = dict(unavailable=repr(e)[:200])
        dt, runs = _timed(lambda: torch_mean(r), a.reps)
        yt, wt = torch_mean(r)
        rec.update(torch_fp64_ms=round(dt * 1e3 + qr_ms, 1), torch_fp64_qr_ms=round(qr_ms, 1), torch_fp64_gram_eigh_ms=round(dt * 1e3, 1),
                   angle_to_torch=_angle(torch, y_solved, yt), weight_err_to_torch=float((fm.weight.double() - wt[:r]).abs().max()))
        if str(n) in a.numpy_n.split(","):
            xs = x.cpu().numpy().astype(np.float64)
            t0 = time.perf_counter()
            qn = np.concatenate([np.linalg.qr(v.T)[0].T for v in xs])
            lam, v = np.linalg.eigh(qn @ qn.T)
            yn = (v[:, -r:][:, ::-1] / np.sqrt(lam[-r:][::-1])).T @ qn
            rec.update(numpy_ms=round((time.perf_counter() - t0) * 1e3, 1), numpy_threads=os.environ.get("OMP_NUM_THREADS", ""),
                       angle_to_numpy=_angle(torch, y_solved, torch.from_numpy(yn).to(DEV)))
        if r == k and str(n) in a.karcher_n.split(","):
            from diffusion_pullback_amd import geometry
            for tag, init in (("member", 0), ("flag", "flag")):
                try:
                    t0 = time.perf_counter()
                    _, fi = geometry.frechet_mean(x, init=init, max_iter=200, tol=1e-6)
                    torch.cuda.synchronize()
                    rec.update({f"karcher_steps_{tag}": fi["iterations"], f"karcher_converged_{tag}": fi["converged"],
                                f"karcher_grad_norm_{tag}": fi["grad_norm"], f"karcher_ms_{tag}": round((time.perf_counter() - t0) * 1e3, 1)})
                except Exception as e:
                    rec[f"karcher_error_{tag}"] = str(e)[:200]
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="16384,32768,81920,196608")
    ap.add_argument("--r", default="10,50")
    ap.add_argument("--b", type=int, default=100)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--max-iter", type=int, default=1000)
    ap.add_argument("--numpy-n", default="16384")
    ap.add_argument("--karcher-n", default="16384")
    ap.add_argument("--seed", type=int, default=97)
    ap.add_argument("--fm-waves", type=int, default=8, help="4: the children run with DPB_FM_WAVES=4, the product kernel's A/B switch")
    ap.add_argument("--leg-timeout", type=int, default=240)
    ap.add_argument("--out", default="")
    ap.add_argument("--leg", default="", help=argparse.SUPPRESS)
    ap.add_argument("--n-one", type=int, default=16384, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return _size_leg(a)
    for n in a.n.split(","):
        cmd = ["timeout", "-k", "10", str(a.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", "size", "--n-one", n, "--b", str(a.b),
               "--k", str(a.k), "--r", a.r, "--reps", str(a.reps), "--steps", str(a.steps), "--max-iter", str(a.max_iter), "--numpy-n", a.numpy_n,
               "--karcher-n", a.karcher_n, "--seed", str(a.seed)]
        r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, DPB_FM_WAVES=str(a.fm_waves)))
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        for ln in lines:
            print(ln, flush=True)
            if a.out:
                with open(a.out, "a") as fh:
                    fh.write(ln + "\n")
        if r.returncode != 0 or not lines:                     # a fault, an abort or a time limit: nothing more is started on the GPU
            print(json.dumps(dict(leg="size", N=int(n), failed=True, returncode=r.returncode, stderr=r.stderr[-800:])), flush=True)
            sys.exit(1)


if __name__ == "__main__":
    main()
