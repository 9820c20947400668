"""Not a test: records what the h-space guidance chain (PullbackUNet.h_space_guidance, dpb_hguide_chain) costs on ONE MI355X in ONE session.
    python tools/gpu_hguide_bench.py [--models ddpm256,sd15] [--dtypes fp32,bf16] [--n 1,4,8] [--steps 0] [--reps 5] [--out profiles/hguide_bench_mi355x.jsonl]
        leg "chain": CelebA-HQ DDPM-256 and SD-v1.5, mid tap, n chains over the DDIM steps of the 100-step table from edit_t = 1.0 to no_edit_t = 0.5
        (--steps K > 0: the first K of those 50 steps): the one chain call against the Python composition it replaces -- per step `forward` at n,
        `forward_shift` at n with xbatch = batch, the scheduler's coefficients and the torch update -- both in the same process, median of `reps`
        device-synchronised calls after a warm-up, with the launches of the chain call and the GEMM flops of one grouped pass against two full passes
        (dpb_engine_stats).  Every (model, dtype) is a child process under its own time limit.
    rocprofv3 --hip-trace --stats -d DIR -o t --output-format csv -- python tools/gpu_hguide_bench.py --leg traced --what chain|composed [--model sd15] [--dtype bf16] [--n 4] [--steps 4] [--calls 3]
        runs `--calls` calls after one warm-up call and nothing else, for the trace.
    python tools/gpu_hguide_bench.py --leg syncs --trace-dir DIR --what chain|composed [--calls 3] [--steps 4] [--out FILE.jsonl]
        reads DIR/**/t_hip_api_trace.csv: the hipStreamSynchronize / hipDeviceSynchronize calls of the whole run (warm-up and engine construction
        included) and, from two such runs with different --calls, per call.
It makes no claim beyond these numbers.  No existing kernel or build line changed with the chain, so there is no headline A/B to run."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCALE = 20.0
TAP = ("mid", 0)


def _setup(model, dtype, n):
    import torch
    from diffusion_pullback_amd import PullbackUNet, configs as cf
    from diffusion_pullback_amd.scheduler import YHCustomScheduler
    dt = {"fp32": torch.float32, "bf16": torch.bfloat16}[dtype]
    g = torch.Generator().manual_seed(0)
    if model == "ddpm256":
        params = cf.ddpm_init_params(cf.CELEBA_HQ_256, seed=0, spectrum=cf.Spectrum())
        net = PullbackUNet("ddpm", cf.CELEBA_HQ_256, params, dtype=dt, device="cuda:0", max_batch=2 * n, max_rank=2, verbose=False)
        ctx, sched = None, YHCustomScheduler(noise_schedule="linear")
    else:
        cfg = cf.sd_config_for("stable-diffusion-v1-5")
        net = PullbackUNet("sd", cfg, cf.sd_init_params(cfg, seed=0), dtype=dt, device="cuda:0", max_batch=2 * n, max_rank=2, verbose=False)
        ctx, sched = torch.randn(n, cfg.ctx_len, cfg.cross_dim, generator=g).cuda(), YHCustomScheduler(noise_schedule="scaled_linear")
    sched.set_timesteps(100)
    x = torch.randn(n, *net.in_shape, generator=g).cuda()
    u = torch.randn(net.engine.tap_numel(TAP), 2, generator=g).cuda()
    return net, sched, x, ctx, u


def _interval(sched, steps):
    e0 = int((sched.timesteps - 1000.0).abs().argmin())
    e1 = int((sched.timesteps - 500.0).abs().argmin())
    return e0, (e1 if steps <= 0 else min(e1, e0 + steps))


def _rows(n):
    return [b % 2 for b in range(n)], [SCALE * (1.0 - 2.0 * (b // 2 % 2)) for b in range(n)]


def _chain(net, sched, x, ctx, u, e0, e1):
    ts, al, an = sched.ddim_triples(e0, e1)
    dirs, scales = _rows(x.shape[0])
    return net.h_space_guidance(x=x, timesteps=ts, alphas=al, alphas_next=an, u=u, dirs=dirs, scales=scales, mode="asyrp", encoder_hidden_states=ctx,
                                op=TAP[0], block_idx=TAP[1], check=False)["states"][:, -1]


def _composed(net, sched, x, ctx, u, e0, e1):
    """what the chain call replaces, step after step: the plain forward at n, the shifted forward at n, the scheduler's coefficients, the update"""
    import torch
    from diffusion_pullback_amd.scheduler import extract
    eng = net.engine
    dirs, scales = _rows(x.shape[0])
    U = (u / u.norm(dim=0, keepdim=True)).T.contiguous()
    for i in range(e0, e1):
        t, tn = sched.timesteps[i], sched.timesteps_next[i]
        e = eng.forward(x, float(t), ctx, "eps")
        es = eng.forward_shift(x, float(t), ctx, TAP, U, dirs, scales, "eps")
        at = extract(sched.alphas_cumprod, t.reshape(()), (1,)).to(x.device).reshape(())
        an = extract(sched.alphas_cumprod, tn.reshape(()), (1,)).to(x.device).reshape(())
        P = (x - es * (1 - at).sqrt()) / at.sqrt()
        x = an.sqrt() * P + (1 - an).sqrt() * e
    return x


def _timed(fn, reps):
    import torch
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def leg_one(a):
    """one (model, dtype): every n"""
    import torch
    ns = [int(v) for v in a.n.split(",")]
    net, sched, xs, ctxs, u = _setup(a.model, a.dtype, max(ns))         # one engine (max_batch = twice the most chains) for every n
    for n in ns:
        x, ctx = xs[:n].contiguous(), None if ctxs is None else ctxs[:n].contiguous()
        e0, e1 = _interval(sched, a.steps)
        with torch.no_grad():
            got, want = _chain(net, sched, x, ctx, u, e0, e1), _composed(net, sched, x, ctx, u, e0, e1)
            agree = float((got - want).abs().max() / want.abs().max())
            c = _timed(lambda: _chain(net, sched, x, ctx, u, e0, e1), a.reps)
            launches = net.engine.stats()[0]
            p = _timed(lambda: _composed(net, sched, x, ctx, u, e0, e1), a.reps)
            eng = net.engine
            dirs, scales = _rows(n)
            U = (u / u.norm(dim=0, keepdim=True)).T.contiguous()
            eng.forward_shift_groups(x, 2, float(sched.timesteps[e0]), ctx, TAP, U, [-1] * n + dirs, [0.0] * n + scales)
            f_grouped = eng.stats()[1]
            eng.forward(x, float(sched.timesteps[e0]), ctx, "eps")
            f_full = eng.stats()[1]
        row = {"leg": "chain", "model": a.model, "dtype": a.dtype, "tap": "mid", "chains": n, "steps": e1 - e0, "reps": a.reps,
               "chain_ms_median": round(c[0], 2), "chain_ms_min_max": [round(c[1], 2), round(c[2], 2)],
               "composed_ms_median": round(p[0], 2), "composed_ms_min_max": [round(p[1], 2), round(p[2], 2)],
               "composed_over_chain": round(p[0] / c[0], 3), "chain_ms_per_step": round(c[0] / (e1 - e0), 3), "chain_launches": launches,
               "gemm_flops_grouped_pass": f_grouped, "gemm_flops_two_full_passes": 2 * f_full, "grouped_over_two_full": round(f_grouped / (2 * f_full), 4),
               "chain_vs_composed_max_rel": agree}
        print(json.dumps(row), flush=True)


def leg_traced(a):
    import torch
    net, sched, x, ctx, u = _setup(a.model, a.dtype, int(a.n.split(",")[0]))
    e0, e1 = _interval(sched, a.steps)
    fn = _chain if a.what == "chain" else _composed
    with torch.no_grad():
        for _ in range(a.calls + 1):
            fn(net, sched, x, ctx, u, e0, e1)
        torch.cuda.synchronize()


def leg_syncs(a, rows):
    hits = glob.glob(os.path.join(a.trace_dir, "**", "*hip_api_trace.csv"), recursive=True)
    if not hits:
        raise SystemExit(f"no hip_api_trace.csv under {a.trace_dir}")
    with open(hits[0]) as fh:
        fn = [r.get("Function", "") for r in csv.DictReader(fh)]
    rows.append({"leg": "syncs", "what": a.what, "model": a.model, "dtype": a.dtype, "chains": int(a.n.split(",")[0]), "steps": a.steps, "calls_after_warm_up": a.calls,
                 "whole_run": {k: fn.count(k) for k in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpyAsync", "hipMemcpy", "hipMemcpyWithStream")}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default="chain", choices=["chain", "one", "traced", "syncs"])
    ap.add_argument("--models", default="ddpm256,sd15")
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--model", default="sd15")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--n", default="1,4,8")
    ap.add_argument("--steps", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--what", default="chain", choices=["chain", "composed"])
    ap.add_argument("--trace-dir", default="")
    ap.add_argument("--limit", type=int, default=420, help="seconds per (model, dtype) child")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = []
    if a.leg == "one":
        return leg_one(a)
    if a.leg == "traced":
        return leg_traced(a)
    if a.leg == "syncs":
        leg_syncs(a, rows)
    else:
        for model in a.models.split(","):
            for dtype in a.dtypes.split(","):
                cmd = [sys.executable, os.path.abspath(__file__), "--leg", "one", "--model", model, "--dtype", dtype, "--n", a.n, "--steps", str(a.steps),
                       "--reps", str(a.reps)]
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
                except subprocess.TimeoutExpired:
                    rows.append({"leg": "chain", "model": model, "dtype": dtype, "status": f"not measured: over the {a.limit} s limit"})
                    print(json.dumps(rows[-1]), flush=True)
                    break                                                # a child that ran out of time: nothing more is started on the device
                got = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
                rows += got
                for g in got:
                    print(json.dumps(g), flush=True)
                if r.returncode != 0:
                    rows.append({"leg": "chain", "model": model, "dtype": dtype, "status": f"child exit {r.returncode}", "stderr_tail": r.stderr[-400:]})
                    print(json.dumps(rows[-1]), flush=True)
                    break                                                # a failed child: nothing more is started on the device
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")
    for r in rows:
        if a.leg == "syncs":
            print(json.dumps(r))


if __name__ == "__main__":
    main()
