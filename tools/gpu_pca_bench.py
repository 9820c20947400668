"""Not a test: times global_pca_zt's two phases at SD-1.5 mid (D = 1280 * 8 * 8 = 81 920) on ONE full-size engine, and the reference's own PCA
on the same features.
    python tools/gpu_pca_bench.py [--dtype bf16] [--n 1000] [--q 100] [--niter 5] [--reps 5] [--ref-reps 3] [--no-ref]
Prints, each as the median of repeats: the feature sampling (dpb_forward per chunk of max_batch = 5 seeded zt straight into H [N][D] fp32,
wall clock, device-synchronised), dpb_pca_lowrank on H (device events), and torch.pca_lowrank(H, q, center=True, niter) on the CPU (the
reference's path at its default pca_device='cpu', same H).  Under `rocprofv3 --kernel-trace --stats` (with --no-ref), the per-kernel times
of the PCA give each product kernel's share of its bound: tools/README.md."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from diffusion_pullback_amd import PullbackUNet, configs as cf  # noqa: E402
from diffusion_pullback_amd.engine import pca_lowrank  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--q", type=int, default=100)
    ap.add_argument("--niter", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-reps", type=int, default=3)
    ap.add_argument("--no-ref", action="store_true", help="skip the CPU torch.pca_lowrank leg (profiling runs)")
    a = ap.parse_args()
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    g = torch.Generator().manual_seed(0)
    net = PullbackUNet("sd", cf.SD15, cf.sd_init_params(cf.SD15, seed=0, spectrum=cf.Spectrum()), dtype=dtype, device="cuda:0", max_batch=5,
                       max_rank=4, verbose=False)
    e = net.engine
    tap = ("mid", 0)
    d = e.tap_numel(tap)
    zt = torch.randn(a.n, 4, 64, 64, generator=g)
    ctx = torch.randn(1, 77, 768, generator=g)
    t = 696.2727
    print(json.dumps(dict(model="sd15", dtype=a.dtype, tap="mid", n=a.n, d=d, q=a.q, niter=a.niter, reps=a.reps, device=torch.cuda.get_device_name(0))),
          flush=True)
    H = torch.empty(a.n, d, dtype=torch.float32, device="cuda:0")

    def sample():
        for i0 in range(0, a.n, e.max_batch):
            b = min(e.max_batch, a.n - i0)
            e.forward(zt[i0:i0 + b], t, ctx, tap, out=H[i0:i0 + b])
    sample()
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        sample()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    print(json.dumps(dict(leg="feature_sampling", median_s=round(statistics.median(ts), 4), runs_s=[round(x, 4) for x in ts],
                          samples_per_s=round(a.n / statistics.median(ts), 1))), flush=True)

    R = torch.randn(min(a.n, d), a.q, generator=torch.Generator().manual_seed(1))
    pca_lowrank(H, R, a.q, a.niter)                        # warm-up: code objects
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        u, s = pca_lowrank(H, R, a.q, a.niter)
        ev1.record()
        ev1.synchronize()
        ms.append(ev0.elapsed_time(ev1))
    n_prod = 2 + 2 * a.niter
    gflop = n_prod * 2.0 * a.q * a.n * d / 1e9
    med = statistics.median(ms)
    print(json.dumps(dict(leg="dpb_pca_lowrank", median_ms=round(med, 3), runs_ms=[round(x, 3) for x in ms], products=n_prod,
                          product_gflop=round(gflop, 1), product_tflops_over_whole_call=round(gflop / med, 2),
                          s_head=[round(x, 3) for x in s[:4].tolist()])), flush=True)
    if not a.no_ref:
        Hc = H.cpu()
        ts = []
        for _ in range(a.ref_reps):
            torch.manual_seed(1)
            t0 = time.perf_counter()
            _, sr, ur = torch.pca_lowrank(Hc, q=a.q, center=True, niter=a.niter)
            ts.append(time.perf_counter() - t0)
        cos = ((u.double().cpu() * ur.T.double()).sum(1).abs() / (u.double().cpu().norm(dim=1) * ur.T.double().norm(dim=1)))
        print(json.dumps(dict(leg="torch_pca_lowrank_cpu", median_s=round(statistics.median(ts), 3), runs_s=[round(x, 3) for x in ts],
                              cpu_threads=torch.get_num_threads(), speedup=round(statistics.median(ts) * 1e3 / med, 1),
                              s_rel_max=float(((s.cpu().double() - sr.double()).abs() / sr.double()).max()),
                              cos_min_top10=float(cos[:10].min()))), flush=True)


if __name__ == "__main__":
    main()
