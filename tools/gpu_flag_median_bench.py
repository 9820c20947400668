"""Not a test: times the flag median (dpb_flag_median_init / _iterate / _round / _finish) on the set of tools/gpu_flag_mean_bench.py with 20 % planted
outliers -- B = 100 local bases of k = 50 Gaussian rows; 80 of them share 10 directions, the other 20 share 10 others; 40 rows of their own each --
at rank r = 10.
    python tools/gpu_flag_median_bench.py [--n 16384,32768,81920,196608] [--r 10] [--reps 3] [--torch-n 16384,32768] [--out FILE.jsonl]
Every size runs in a fresh child process under its own time limit (--leg-timeout seconds); the first that fails or runs out of time ends the run.  One
JSON line per N, appended to --out as well; times are device-synchronised wall clock, all in one session:
  init_ms               dpb_flag_median_init (the cross-Gram pass over X, the whitening, the start block, the table), median of --reps
  rounds, converged, objective   the run of geometry.flag_median's loop at its defaults (eps 1e-5, tol 1e-9, inner tol 1e-12, status read every 16)
  inner_iterations      per round: the first is the cold solve of the flag mean, the later ones are warm-started at the previous round's block
  inner_ms, round_ms    per round: the inner solve (its status reads included) and the round step (Rayleigh-Ritz, the unweighted pass M = Ghat C^T,
                        affinities, objective, the new table; its one host read included)
  finish_ms             dpb_flag_median_finish, median of --reps
  cold_mean_iterations  dpb_flag_mean_*'s iterations on the same set: what every round would cost without the warm start
  kernels               device time per launch (torch.profiler) of fmw_product_kernel (the weighted pass D Ghat D Z) beside fm_product_kernel (the
                        unweighted pass) on the same Ghat and the same block width in the same process, with their GB/s of Ghat
  torch_fp64_ms         sizes of --torch-n: the float64 torch composition of the reference on the same GPU (batched qr once; per round the Gram of
                        the scaled rows, eigh, the top r rows, the distances), rounds_torch and angle_to_torch (largest principal angle, float64)"""
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


def _sync_ms(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _set(b, k, n, shared=10, outliers=0.2, seed=97):
    import torch
    g = torch.Generator(device=DEV).manual_seed(seed)
    common = torch.randn(shared, n, generator=g, device=DEV)
    other = torch.randn(shared, n, generator=g, device=DEV)
    x = torch.randn(b, k, n, generator=g, device=DEV)
    n_out = int(round(outliers * b))
    x[:b - n_out, :shared] = common
    x[b - n_out:, :shared] = other
    return x, n_out


class _Median:
    def __init__(self, x, r, cap):
        import torch
        from diffusion_pullback_amd import geometry
        from diffusion_pullback_amd import lib as L
        self.L, self.lib, self.x, self.r, self.cap, self.head = L, L.load(), x, r, cap, geometry._median_head
        self.b, self.k, self.n = x.shape
        self.need = int(self.lib.dpb_flag_median_scratch_bytes(self.b, self.k, self.n, r, cap))
        assert self.need > 0
        self.scratch = torch.empty(self.need, dtype=torch.uint8, device=DEV)
        self.st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.Y = torch.empty(r, self.n, device=DEV)
        self.weight = torch.empty(r, device=DEV)
        self.theta = torch.empty(self.b, min(r, self.k), device=DEV)
        self.Ct = torch.empty(self.b * self.k, r, dtype=torch.float64, device=DEV)
        self.member = torch.empty(3, self.b, dtype=torch.float64, device=DEV)
        self.info = torch.empty(72 + self.b, dtype=torch.float64, device=DEV)

    def args(self):
        return self.b, self.k, self.n, self.r, self.cap, self.scratch.data_ptr(), self.need, self.st

    def init(self):
        self.L.check(self.lib.dpb_flag_median_init(self.x.data_ptr(), None, None, self.b, self.k, self.n, self.r, 0, self.cap, self.scratch.data_ptr(),
                                                   self.need, self.st))

    def iterate(self, steps, tol):
        self.L.check(self.lib.dpb_flag_median_iterate(steps, tol, None, *self.args()))

    def inner(self, tol=1e-12, every=16):
        asked = 0
        while asked < self.cap:
            steps = min(every, self.cap - asked)
            self.iterate(steps, tol)
            asked += steps
            if self.head(self.scratch)["done"] != 0:
                break

    def round(self, eps, tol, update):
        self.L.check(self.lib.dpb_flag_median_round(eps, tol, 1 if update else 0, None, *self.args()))
        return self.head(self.scratch)

    def finish(self):
        self.L.check(self.lib.dpb_flag_median_finish(self.x.data_ptr(), None, self.Y.data_ptr(), self.weight.data_ptr(), self.theta.data_ptr(),
                                                     self.Ct.data_ptr(), self.member.data_ptr(), self.info.data_ptr(), *self.args()))


def _angle(torch, ya, yb):
    qa = torch.linalg.qr(ya.double().T).Q
    qb = torch.linalg.qr(yb.double().T).Q
    return float(torch.asin(torch.linalg.svdvals(qa - qb @ (qb.T @ qa)).max().clamp(max=1.0)))


def _kernel_pair(torch, med, x, r, cap, steps):
    """device time per launch of the weighted and the unweighted product kernel, `steps` iterations each on the same Ghat, one traced run"""
    from torch.profiler import ProfilerActivity, profile
    lib, L = med.lib, med.L
    b, k, n = x.shape
    need = int(lib.dpb_flag_mean_scratch_bytes(b, k, n, r, cap))
    fs = torch.empty(need, dtype=torch.uint8, device=DEV)
    L.check(lib.dpb_flag_mean_init(x.data_ptr(), None, b, k, n, r, 0, cap, fs.data_ptr(), need, med.st))
    med.init()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        med.iterate(steps, 0.0)
        L.check(lib.dpb_flag_mean_iterate(steps, 0.0, None, b, k, n, r, cap, fs.data_ptr(), need, med.st))
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        key = "fmw_product" if "fmw_product_kernel" in ev.key else "fm_product" if "fm_product_kernel" in ev.key else None
        if key:
            total = getattr(ev, "device_time_total", None)
            total = ev.cuda_time_total if total is None else total
            us = total / ev.count
            out[key] = dict(us_per_launch=round(us, 2), launches=ev.count, ghat_gbytes_per_s=round(8.0 * (b * k) ** 2 / (us * 1e-6) / 1e9, 1))
    return out


def _torch_median(torch, x, r, eps, tol, max_rounds):
    b, k, n = x.shape
    q = torch.linalg.qr(x.double().transpose(1, 2)).Q.transpose(1, 2)                      # [B, k, N]
    w = torch.ones(b, dtype=torch.float64, device=DEV)
    hist = []
    while True:
        s = (w.sqrt()[:, None, None] * q).reshape(b * k, n)
        lam, v = torch.linalg.eigh(s @ s.T)
        y = (v[:, -r:].flip(1) / lam[-r:].flip(0).sqrt()).T @ s
        d = (r - (q @ y.T).square().sum(dim=(1, 2))).clamp(min=0).sqrt()
        hist.append(float(torch.where(d >= eps, d, d * d / (2 * eps) + eps / 2).sum()))
        if len(hist) >= 2 and hist[-2] - hist[-1] <= tol * hist[-2]:
            break
        if len(hist) > max_rounds:
            break
        w = 1.0 / d.clamp(min=eps)
        w = w * b / w.sum()
    return y, hist


def _size_leg(a):
    import torch
    b, k, n, r = a.b, a.k, a.n_one, a.r
    x, n_out = _set(b, k, n, seed=a.seed)
    med = _Median(x, r, a.inner_iter)
    rec = dict(leg="size", B=b, k=k, N=n, r=r, R=b * k, outliers=n_out, seed=a.seed, eps=a.eps, tol=a.tol,
               fm_waves=int(os.environ.get("DPB_FM_WAVES", "8")), ghat_gbytes=round(8.0 * (b * k) ** 2 / 1e9, 3))
    med.init()
    rec["init_ms"] = round(statistics.median(_sync_ms(med.init)[0] for _ in range(a.reps)), 3)
    objective, inner_its, inner_ms, round_ms, converged = [], [], [], [], False
    while True:
        inner_ms.append(round(_sync_ms(med.inner)[0], 3))
        update = len(objective) < a.max_rounds
        dt, head = _sync_ms(lambda: med.round(a.eps, a.tol, update))
        round_ms.append(round(dt, 3))
        objective.append(head["J"])
        inner_its.append(head["iters"])
        converged = head["converged"]
        if converged or not update or head["done"] == 2:
            break
    med.finish()
    rec["finish_ms"] = round(statistics.median(_sync_ms(med.finish)[0] for _ in range(a.reps)), 3)
    mw = med.member[2].cpu()
    rec.update(rounds=len(objective) - 1, converged=bool(converged), objective=objective, inner_iterations=inner_its, inner_ms=inner_ms,
               round_ms=round_ms, total_ms=round(rec["init_ms"] + sum(inner_ms) + sum(round_ms) + rec["finish_ms"], 3),
               inlier_weight_min=float(mw[:b - n_out].min()), outlier_weight_max=float(mw[b - n_out:].max()) if n_out else None)
    y_med = med.Y.clone()
    from diffusion_pullback_amd import geometry
    _, fi = geometry.flag_mean(x, rank=r, max_iter=a.inner_iter)
    rec["cold_mean_iterations"] = fi["iterations"]
    try:
        rec["kernels"] = _kernel_pair(torch, med, x, r, a.inner_iter, a.steps)
    except Exception as e:                                     # the profiler is a convenience: the times above stand without it
        rec["kernels"] = dict(unavailable=repr(e)[:200])
    if str(n) in a.torch_n.split(","):
        _torch_median(torch, x, r, a.eps, a.tol, 1)            # warm-up
        dt, (yt, hist) = _sync_ms(lambda: _torch_median(torch, x, r, a.eps, a.tol, a.max_rounds))
        rec.update(torch_fp64_ms=round(dt, 1), rounds_torch=len(hist) - 1, angle_to_torch=_angle(torch, y_med, yt),
                   objective_err_to_torch=abs(hist[-1] - objective[-1]) / hist[-1])
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="16384,32768,81920,196608")
    ap.add_argument("--r", type=int, default=10)
    ap.add_argument("--b", type=int, default=100)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--inner-iter", type=int, default=200)
    ap.add_argument("--max-rounds", type=int, default=50)
    ap.add_argument("--eps", type=float, default=1e-5)
    ap.add_argument("--tol", type=float, default=1e-9)
    ap.add_argument("--torch-n", default="16384,32768")
    ap.add_argument("--seed", type=int, default=97)
    ap.add_argument("--fm-waves", type=int, default=8, help="4: the children run with DPB_FM_WAVES=4, the product kernels' A/B switch")
    ap.add_argument("--leg-timeout", type=int, default=240)
    ap.add_argument("--out", default="")
    ap.add_argument("--leg", default="", help=argparse.SUPPRESS)
    ap.add_argument("--n-one", type=int, default=16384, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return _size_leg(a)
    for n in a.n.split(","):
        cmd = ["timeout", "-k", "10", str(a.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", "size", "--n-one", n, "--b", str(a.b),
               "--k", str(a.k), "--r", str(a.r), "--reps", str(a.reps), "--steps", str(a.steps), "--inner-iter", str(a.inner_iter), "--max-rounds",
               str(a.max_rounds), "--eps", str(a.eps), "--tol", str(a.tol), "--torch-n", a.torch_n, "--seed", str(a.seed)]
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
