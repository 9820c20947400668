"""Not a test: times the three phases of local_pca_zt / local_pca_xt on ONE full-size engine, against what the parent commit could compose.
    python tools/gpu_local_pca_bench.py [--model sd15|ddpm256] [--dtype bf16] [--n 5000] [--q 100] [--reps 5] [--no-ref] [--overlap]
Prints one JSON line per leg, each the median of --reps runs (wall clock, device-synchronised):
  sampling            dpb_local_pca_sample: perturbation + forward per chunk of max_batch = 5 on the device, features straight into H [N][D]
  sampling_composed   the yardstick: torch.randn_like + normalise + add on the device, then eng.forward per chunk (same max_batch)
  pca                 dpb_pca_lowrank(H, q, niter = 2)
  x_directions        inv_jac_zt of the q columns (one primal, adjoints in chunks of max_rank)
  torch_pca_lowrank_cpu  the reference's PCA on the same H (skipped with --no-ref or above --ref-max-n samples)
  bf16_vs_fp32_overlap   with --overlap: ||U32^T U16||_F^2 / q of the top-q bases of a bf16 and an fp32 engine under the same seed and R
SD-1.5 runs at the headline's null conditioning (zeros [1, 77, 768])."""
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

DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def _net(model, dtype, max_rank):
    if model == "sd15":
        return PullbackUNet("sd", cf.SD15, cf.sd_init_params(cf.SD15, seed=0, spectrum=cf.Spectrum()), dtype=dtype, device="cuda:0", max_batch=5,
                            max_rank=max_rank, verbose=False)
    return PullbackUNet("ddpm", cf.CELEBA_HQ_256, cf.ddpm_init_params(cf.CELEBA_HQ_256, seed=0, spectrum=cf.Spectrum()), dtype=dtype, device="cuda:0",
                        max_batch=5, max_rank=max_rank, verbose=False)


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), [round(x, 4) for x in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="sd15", choices=["sd15", "ddpm256"])
    ap.add_argument("--dtype", default="bf16", choices=list(DT))
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--q", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-rank", type=int, default=50)
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--ref-max-n", type=int, default=5000)
    ap.add_argument("--overlap", action="store_true")
    a = ap.parse_args()
    net = _net(a.model, DT[a.dtype], a.max_rank)
    e, tap = net.engine, ("mid", 0)
    d = e.tap_numel(tap)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, *net.in_shape, generator=g).to("cuda:0")
    ctx = torch.zeros(1, 77, 768, device="cuda:0") if a.model == "sd15" else None
    t = 696.2727
    print(json.dumps(dict(model=a.model, dtype=a.dtype, tap="mid", n=a.n, d=d, q=a.q, niter=2, reps=a.reps, max_batch=e.max_batch,
                          max_rank=a.max_rank, device=torch.cuda.get_device_name(0))), flush=True)
    H = torch.empty(a.n, d, dtype=torch.float32, device="cuda:0")

    def composed():
        for i0 in range(0, a.n, e.max_batch):
            b = min(e.max_batch, a.n - i0)
            eps = torch.randn(b, *net.in_shape, device="cuda:0")
            xb = x + eps / eps.view(b, -1).norm(dim=-1).view(b, 1, 1, 1)
            e.forward(xb, t, ctx, tap, out=H[i0:i0 + b])
    med_c, runs = _timed(composed, a.reps)
    print(json.dumps(dict(leg="sampling_composed", median_s=round(med_c, 4), runs_s=runs, samples_per_s=round(a.n / med_c, 1))), flush=True)
    med, runs = _timed(lambda: e.local_pca_sample(x, t, ctx, tap, a.n, seed=1, out=H), a.reps)
    print(json.dumps(dict(leg="sampling", median_s=round(med, 4), runs_s=runs, samples_per_s=round(a.n / med, 1),
                          composed_over_this=round(med_c / med, 3))), flush=True)
    R = torch.randn(min(a.n, d), a.q, generator=torch.Generator().manual_seed(1))
    out = {}

    def pca():
        out["u"], out["s"] = pca_lowrank(H, R, a.q, 2)
    med_p, runs = _timed(pca, a.reps)
    print(json.dumps(dict(leg="pca", median_s=round(med_p, 4), runs_s=runs, s_head=[round(v, 4) for v in out["s"][:4].tolist()])), flush=True)
    u, s = out["u"], out["s"]
    med_x, runs = _timed(lambda: net.inv_jac_zt(x, t, ctx, op="mid", block_idx=0, u=u.T), a.reps)
    print(json.dumps(dict(leg="x_directions", median_s=round(med_x, 4), runs_s=runs)), flush=True)
    if not a.no_ref and a.n <= a.ref_max_n:
        Hc = H.cpu()
        ts = []
        for _ in range(3):
            torch.manual_seed(1)
            t0 = time.perf_counter()
            _, sr, ur = torch.pca_lowrank(Hc, q=a.q, center=True, niter=2)
            ts.append(time.perf_counter() - t0)
        print(json.dumps(dict(leg="torch_pca_lowrank_cpu", median_s=round(statistics.median(ts), 3), runs_s=[round(v, 3) for v in ts],
                              cpu_threads=torch.get_num_threads(), over_device_pca=round(statistics.median(ts) / med_p, 1),
                              s_rel_max=float(((s.cpu().double() - sr.double()).abs() / sr.double()).max()))), flush=True)
    if a.overlap:
        del net, e
        bases = {}
        for name in ("fp32", "bf16"):
            nn = _net(a.model, DT[name], 4)
            Hh = nn.engine.local_pca_sample(x, t, ctx, tap, a.n, seed=1, out=H)
            bases[name] = pca_lowrank(Hh, R, a.q, 2)[0].double()
            del nn
        ov = (bases["fp32"] @ bases["bf16"].T).pow(2).sum().item() / a.q
        print(json.dumps(dict(leg="bf16_vs_fp32_overlap", n=a.n, q=a.q, overlap=round(ov, 4))), flush=True)


if __name__ == "__main__":
    main()
