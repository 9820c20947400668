"""Not a test: times the fused decoder iterate (dpb_pullback_iterate_between: V <- orth(J_dec^T J_dec V), J_dec = d eps / d h at the mid
tap) next to the same-session encoder headline (dpb_pullback_iterate at mid) on ONE full-size engine.
    python tools/gpu_decoder_bench.py [--dtype bf16] [--k 5] [--iters 10] [--reps 7] [--ddpm]
Prints per leg: iterations/s (median of `reps` timed windows of `iters` fused iterations each, device-synchronised), the dpb_engine_stats of
one iteration (launches, algorithmic GEMM flops; the tangent and adjoint passes together), and that flop count's rate as a share of the
dense 16-bit MFMA peak (2.5 PFLOP/s; fp32: 157.3 TFLOP/s) -- a whole-iteration figure, not a kernel's share."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from diffusion_pullback_amd import PullbackUNet, configs as cf  # noqa: E402

PEAK = {torch.bfloat16: 2.5e15, torch.float16: 2.5e15, torch.float32: 157.3e12}


def timed(fn, iters, reps):
    fn(2)                                                 # warm-up: code objects, GEMM plans
    torch.cuda.synchronize()
    rates = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn(iters)
        torch.cuda.synchronize()
        rates.append(iters / (time.perf_counter() - t0))
    return statistics.median(rates), rates


def leg(net, name, run, iters, reps, dtype):
    med, rates = timed(run, iters, reps)
    launches, flops, _ = net.engine.stats()              # the last call: `iters` iterations
    per_it = flops / iters
    out = dict(leg=name, iterations_per_s=round(med, 2), rates=[round(r, 2) for r in rates], launches_per_iteration=launches // iters,
               gemm_gflop_per_iteration=round(per_it / 1e9, 1), mfma_peak_share=round(per_it * med / PEAK[dtype], 4))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ddpm", action="store_true", help="CelebA-HQ DDPM-256 instead of SD-1.5")
    a = ap.parse_args()
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    g = torch.Generator().manual_seed(0)
    if a.ddpm:
        cfg = cf.CELEBA_HQ_256
        net = PullbackUNet("ddpm", cfg, cf.ddpm_init_params(cfg, seed=0, spectrum=cf.Spectrum()), dtype=dtype, device="cuda:0", max_batch=1,
                           max_rank=a.k, verbose=False)
        x, t, ctx, model = torch.randn(1, 3, 256, 256, generator=g), 600.0, None, "ddpm256"
    else:
        net = PullbackUNet("sd", cf.SD15, cf.sd_init_params(cf.SD15, seed=0, spectrum=cf.Spectrum()), dtype=dtype, device="cuda:0", max_batch=1,
                           max_rank=a.k, verbose=False)
        x, t, ctx, model = torch.randn(1, 4, 64, 64, generator=g), 696.2727, torch.randn(1, 77, 768, generator=g), "sd15"
    e = net.engine
    tap = ("mid", 0)
    n_h, n_x = e.tap_numel(tap), e.n_in
    print(json.dumps(dict(model=model, dtype=a.dtype, k=a.k, tap="mid", n_h=n_h, n_x=n_x, iters=a.iters, reps=a.reps,
                          device=torch.cuda.get_device_name(0))), flush=True)
    e.primal(x, t, ctx, "eps")                            # one primal serves both legs (it covers the whole tape)
    Vd = torch.linalg.qr(torch.randn(n_h, a.k, generator=g))[0].T.contiguous().cuda()
    Ve = torch.linalg.qr(torch.randn(n_x, a.k, generator=g))[0].T.contiguous().cuda()
    scratch = torch.empty(e.scratch_bytes(tap, a.k) + 256, dtype=torch.uint8, device="cuda:0")
    res = []
    for _ in range(2):                                   # alternate the legs: encoder, decoder, encoder, decoder
        res.append(leg(net, "encoder_mid", lambda n: e.iterate(tap, Ve, n), a.iters, a.reps, dtype))
        res.append(leg(net, "decoder_mid", lambda n: e.iterate_between(tap, "eps", Vd, n, scratch), a.iters, a.reps, dtype))
    enc = statistics.median([r["iterations_per_s"] for r in res if r["leg"] == "encoder_mid"])
    dec = statistics.median([r["iterations_per_s"] for r in res if r["leg"] == "decoder_mid"])
    print(json.dumps(dict(summary=model, dtype=a.dtype, k=a.k, encoder_iterations_per_s=enc, decoder_iterations_per_s=dec,
                          decoder_over_encoder_time=round(enc / dec, 2))), flush=True)


if __name__ == "__main__":
    main()
