"""Not a test: times one sweep of the Hungarian-matched mean (dpb_matched_mean, csrc/hungarian.hip) at the sizes of the global-basis job, B = 100 local
bases of k = 50 rows.
    python tools/gpu_hungarian_bench.py [--n 16384,32768,81920,196608] [--b 100] [--k 50] [--reps 5] [--out FILE.jsonl]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/gpu_hungarian_bench.py --leg sweeps --n-one 16384 --sweeps 10
    python tools/gpu_hungarian_bench.py --leg split --stats DIR/.../t_kernel_stats.csv --sweeps 10 --n-one 16384 [--out FILE.jsonl]
N: 16 384 (SD x), 81 920 (SD h), 32 768 and 196 608 (DDPM h and x).  The set: per basis 10 directions shared by all (plus half their norm of noise) and
40 of its own, Gaussian rows.  Every size runs in a fresh child process under its own time limit (--leg-timeout seconds); the first that fails or runs
out of time ends the run.  One JSON line per size, appended to --out as well; every time is the median of --reps after a warm-up, device-synchronised:
  copy_gbytes_per_s     a device-to-device copy of the bytes of X (read plus written over its time), IN THIS RUN: the bound of the mean pass
  sweep_ms              one dpb_matched_mean call (anchor X[0])
  overlap_ms            its overlap pass alone, through the public entry points it is made of: dpb_cross_gram(anchor, X) and the two dpb_row_sumsq
  assign_ms             dpb_linear_assignment on the sweep's own 100 cost matrices (the same kernel; in the sweep it forms the cost while loading)
  assign_k128_ms        the same on 100 uniform-random 128 x 128 matrices;  scipy_ms / scipy_k128_ms: scipy.optimize.linear_sum_assignment over the
                        same matrices on the host, one after another
  mean_ms               sweep_ms - overlap_ms - assign_ms (the streaming pass and its normalisation, by difference; the split leg measures it directly),
                        mean_x_gbytes_per_s: the bytes of X over it, and its share of the copy's rate
  torch_fp64_sweep_ms   the float64 torch composition on the same GPU: matmul against the unit rows -> cost -> host scipy -> gather -> sum -> normalise
                        (torch_fp64_setup_ms: the unit rows in float64, once)
  agreement             entries of perm / sign that differ from the composition's (scipy's), the largest relative gap of a basis's assignment cost to
                        scipy's optimum on the composition's matrix, and the largest |Y - Y_ref| in units of the bar 2^-23 |Y_ref| + 1e-12, Y_ref the
                        float64 mean under the device's perm / sign
The split of a sweep into its kernels comes from a rocprofv3 run of its own (legs `sweeps` and `split` above)."""
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


def _host_timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def _set(b, k, n, shared=10, seed=97):
    import torch
    g = torch.Generator(device=DEV).manual_seed(seed)
    common = torch.randn(shared, n, generator=g, device=DEV)
    x = torch.randn(b, k, n, generator=g, device=DEV)
    x[:, :shared] = common + 0.5 * x[:, :shared]
    return x


class _Sweep:
    """dpb_matched_mean and the public pieces of its overlap pass on the same buffers"""

    def __init__(self, x):
        import torch
        from diffusion_pullback_amd import lib as L
        self.L, self.lib, self.x = L, L.load(), x
        self.b, self.k, self.n = x.shape
        self.need = int(self.lib.dpb_matched_mean_scratch_bytes(self.b, self.k, self.n))
        assert self.need > 0
        self.scratch = torch.empty(self.need, dtype=torch.uint8, device=DEV)
        self.st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.Y = torch.empty(self.k, self.n, device=DEV)
        self.perm = torch.full((self.b, self.k), -1, dtype=torch.int32, device=DEV)
        self.sign = torch.zeros(self.b, self.k, dtype=torch.int32, device=DEV)
        self.info = torch.empty(1 + 2 * self.b, dtype=torch.float64, device=DEV)
        self.G = torch.empty(self.k, self.b * self.k, dtype=torch.float64, device=DEV)
        self.ss = torch.empty(self.b * self.k + self.k, dtype=torch.float64, device=DEV)

    def sweep(self):
        self.L.check(self.lib.dpb_matched_mean(self.x.data_ptr(), self.b, self.k, self.n, None, 0, 0, self.Y.data_ptr(), self.perm.data_ptr(),
                                               self.sign.data_ptr(), self.info.data_ptr(), self.scratch.data_ptr(), self.need, self.st))

    def overlap(self):
        r = self.b * self.k
        self.L.check(self.lib.dpb_cross_gram(self.x.data_ptr(), self.x.data_ptr(), self.G.data_ptr(), self.k, r, self.n, self.st))
        self.L.check(self.lib.dpb_row_sumsq(self.x.data_ptr(), self.k, self.n, self.ss[r:].data_ptr(), self.st))
        self.L.check(self.lib.dpb_row_sumsq(self.x.data_ptr(), r, self.n, self.ss.data_ptr(), self.st))

    def cost(self):
        """[B, k, k] float64: the '1/cosine' matrices of the sweep, from the overlap buffers"""
        r = self.b * self.k
        c = self.G.view(self.k, self.b, self.k) / (self.ss[r:].sqrt()[:, None, None] * self.ss[:r].sqrt().view(1, self.b, self.k))
        return (1.0 / c.abs().clamp(min=2.0 ** -40)).permute(1, 0, 2).contiguous()


def _scipy_all(costs):
    from scipy.optimize import linear_sum_assignment
    return [linear_sum_assignment(m)[1] for m in costs]


def _size_leg(a):
    import numpy as np
    import torch
    from diffusion_pullback_amd import geometry
    b, k, n = a.b, a.k, a.n_one
    rec = dict(leg="size", B=b, k=k, N=n, seed=a.seed, x_gbytes=round(4.0 * b * k * n / 1e9, 3))
    x = _set(b, k, n, seed=a.seed)
    dst = torch.empty_like(x)
    dt, _ = _timed(lambda: dst.copy_(x), a.reps)
    copy_rate = 2.0 * x.numel() * 4 / dt / 1e9
    rec["copy_gbytes_per_s"] = round(copy_rate, 1)
    del dst
    m = _Sweep(x)
    dt_sweep, runs = _timed(m.sweep, a.reps)
    rec.update(sweep_ms=round(dt_sweep * 1e3, 3), sweep_ms_runs=runs)
    dt_ov, runs = _timed(m.overlap, a.reps)
    rec.update(overlap_ms=round(dt_ov * 1e3, 3), overlap_ms_runs=runs, overlap_x_gbytes_per_s=round(4.0 * b * k * n / dt_ov / 1e9, 1))
    cost = m.cost()
    dt_as, runs = _timed(lambda: geometry.linear_assignment(cost), a.reps)
    cost_h = cost.cpu().numpy()
    rec.update(assign_ms=round(dt_as * 1e3, 3), assign_ms_runs=runs, scipy_ms=round(_host_timed(lambda: _scipy_all(cost_h), a.reps) * 1e3, 3))
    big = torch.rand(b, 128, 128, dtype=torch.float64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(a.seed))
    dt_big, _ = _timed(lambda: geometry.linear_assignment(big), a.reps)
    big_h = big.cpu().numpy()
    rec.update(assign_k128_ms=round(dt_big * 1e3, 3), scipy_k128_ms=round(_host_timed(lambda: _scipy_all(big_h), a.reps) * 1e3, 3))
    dt_mean = dt_sweep - dt_ov - dt_as
    rec.update(mean_ms=round(dt_mean * 1e3, 3), mean_x_gbytes_per_s=round(4.0 * b * k * n / max(dt_mean, 1e-9) / 1e9, 1),
               mean_share_of_copy=round(4.0 * b * k * n / max(dt_mean, 1e-9) / 1e9 / copy_rate, 3))

    # the float64 torch composition of one sweep
    t0 = time.perf_counter()
    xh = x.double()
    xh = xh / xh.norm(dim=2, keepdim=True)
    torch.cuda.synchronize()
    rec["torch_fp64_setup_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    state = {}

    def torch_sweep():
        c = torch.einsum("in,bjn->bij", xh[0], xh)
        d = (1.0 / c.abs().clamp(min=2.0 ** -40)).cpu().numpy()
        perm = torch.from_numpy(np.stack(_scipy_all(d))).to(DEV)
        sg = torch.where(c.gather(2, perm[:, :, None])[:, :, 0] < 0, -1.0, 1.0).double()
        s = (sg[:, :, None] * xh.gather(1, perm[:, :, None].expand(-1, -1, n))).sum(dim=0)
        state.update(perm=perm, sign=sg, d=d, Y=s / s.norm(dim=1, keepdim=True))
    dt, runs = _timed(torch_sweep, a.reps)
    rec.update(torch_fp64_sweep_ms=round(dt * 1e3, 3), torch_fp64_sweep_ms_runs=runs)

    # agreement
    m.perm.fill_(-1); m.sign.zero_()
    m.sweep()
    perm, sign = m.perm.long(), m.sign
    own = np.array([state["d"][i][np.arange(k), perm[i].cpu().numpy()].sum() for i in range(b)])
    best = np.array([state["d"][i][np.arange(k), state["perm"][i].cpu().numpy()].sum() for i in range(b)])
    s = (sign.double()[:, :, None] * xh.gather(1, perm[:, :, None].expand(-1, -1, n))).sum(dim=0)
    yr = s / s.norm(dim=1, keepdim=True)
    rec["agreement"] = dict(perm_entries_differing=int((perm != state["perm"]).sum()), sign_entries_differing=int((sign.double() != state["sign"]).sum()),
                            cost_gap_relative=float(np.abs(own - best).max() / np.abs(best).max()),
                            y_error_in_bars=float(((m.Y.double() - yr).abs() / (2.0 ** -23 * yr.abs() + 1e-12)).max()),
                            changed=float(m.info[0]), degenerate=int((m.info[1 + b:] != 0).sum()))
    print(json.dumps(rec), flush=True)


def _sweeps_leg(a):
    """the work a kernel trace is taken of: the first sweep (anchor X[0]), --sweeps times"""
    import torch
    m = _Sweep(_set(a.b, a.k, a.n_one, seed=a.seed))
    for _ in range(a.sweeps):
        m.sweep()
    torch.cuda.synchronize()


def _split_leg(a):
    rows = list(csv.DictReader(open(a.stats)))
    fam = dict(cross_gram=0.0, rowsumsq=0.0, assignment=0.0, mean_stream=0.0, mean_finish=0.0, other=0.0)
    for r in rows:
        name, ns = r["Name"], float(r["TotalDurationNs"])
        key = ("cross_gram" if "cross_gram_kernel" in name else "rowsumsq" if "rowsumsq_kernel" in name else "assignment" if "lap_kernel" in name else
               "mean_stream" if "mean_kernel" in name else "mean_finish" if ("finish_kernel" in name or "changed_kernel" in name) else "other")
        fam[key] += ns
    per = lambda key: round(fam[key] / 1e6 / a.sweeps, 4)
    xb = 4.0 * a.b * a.k * a.n_one
    rec = dict(leg="split", B=a.b, k=a.k, N=a.n_one, sweeps=a.sweeps, source="rocprofv3 --kernel-trace --stats", cross_gram_ms=per("cross_gram"),
               rowsumsq_ms=per("rowsumsq"), assignment_ms=per("assignment"), mean_stream_ms=per("mean_stream"), mean_finish_ms=per("mean_finish"),
               mean_stream_x_gbytes_per_s=round(xb * a.sweeps / max(fam["mean_stream"], 1.0), 1),
               kernel_ms_per_sweep=round(sum(v for k_, v in fam.items() if k_ != "other") / 1e6 / a.sweeps, 4))
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="16384,32768,81920,196608")
    ap.add_argument("--b", type=int, default=100)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=97)
    ap.add_argument("--leg-timeout", type=int, default=240)
    ap.add_argument("--out", default="")
    ap.add_argument("--stats", default="")
    ap.add_argument("--leg", default="", help=argparse.SUPPRESS)
    ap.add_argument("--n-one", type=int, default=16384, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return {"size": _size_leg, "sweeps": _sweeps_leg, "split": _split_leg}[a.leg](a)
    for n in a.n.split(","):
        cmd = ["timeout", "-k", "10", str(a.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", "size", "--n-one", n, "--b", str(a.b),
               "--k", str(a.k), "--reps", str(a.reps), "--seed", str(a.seed)]
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
