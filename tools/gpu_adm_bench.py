"""Not a test: records the speed of the guided-diffusion (ADM) kind next to the DDPM kind, on ONE MI355X in ONE session.
    python tools/gpu_adm_bench.py [--k 5] [--iters 10] [--reps 5] [--out profiles/adm_bench_p2_256_mid_k5.jsonl]
Per leg -- ADM-P2-256 (configs.ADM_P2_256) and the CelebA-HQ DDPM-256 config, each at the mid tap in fp32 and bf16, upto=('mid', 0) -- one JSON
line: iterations/s of the fused power iteration (dpb_pullback_iterate: median of `reps` timed windows of `iters` iterations, device-synchronised)
and the dpb_engine_stats of one iteration (launches, algorithmic GEMM flops).  It makes no claim beyond these numbers.  The same-session
headline A/B against a parent build (the GroupNorm kernels gained an argument) is tools/ab_env.sh with DPB_LIB:
    bash tools/ab_env.sh adm_headline "DPB_LIB=<parent libdpb.so>" "DPB_LIB=diffusion_pullback_amd/libdpb.so"   -> profiles/adm_headline_ab.txt"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from diffusion_pullback_amd import PullbackUNet, configs as cf  # noqa: E402


def leg(name, kind, cfg, params, dtype, k, iters, reps):
    net = PullbackUNet(kind, cfg, params, dtype=dtype, device="cuda:0", max_batch=1, max_rank=k, upto=("mid", 0), verbose=False)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, *net.in_shape, generator=g)
    V0 = torch.linalg.qr(torch.randn(x[0].numel(), k, generator=g))[0].T.contiguous()
    run = lambda n: net.pullback_fixed(x, 600.0, None, "mid", 0, k, n, V0)
    run(2)
    torch.cuda.synchronize()
    rates = []
    for _ in range(reps):
        t0 = time.perf_counter()
        _, s, _, _ = run(iters)
        torch.cuda.synchronize()
        rates.append(iters / (time.perf_counter() - t0))
    launches, flops, _ = net.engine.stats()              # the last call: `iters` iterations
    out = dict(leg=name, dtype=str(dtype).split(".")[-1], k=k, iterations_per_s=round(statistics.median(rates), 2), rates=[round(r, 2) for r in rates],
               launches_per_iteration=launches // iters, gemm_gflop_per_iteration=round(flops / iters / 1e9, 1), s=[round(v, 3) for v in s.tolist()])
    print(json.dumps(out), flush=True)
    del net
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = []
    adm = cf.adm_init_params(cf.ADM_P2_256, seed=0, spectrum=cf.Spectrum())
    ddpm = cf.ddpm_init_params(cf.CELEBA_HQ_256, seed=0, spectrum=cf.Spectrum())
    for dtype in (torch.float32, torch.bfloat16):
        rows.append(leg("adm_p2_256_mid", "adm", cf.ADM_P2_256, adm, dtype, a.k, a.iters, a.reps))
        rows.append(leg("ddpm256_mid", "ddpm", cf.CELEBA_HQ_256, ddpm, dtype, a.k, a.iters, a.reps))
    if a.out:
        with open(a.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
