"""Not a test: records what the newton-h chain (PullbackUNet.newton_h_chain, dpb_newton_h_chain) costs and buys on ONE MI355X in ONE session.
    python tools/gpu_newton_h_bench.py [--n 1,4,8] [--steps 4] [--iters 8] [--reps 5] [--out profiles/newton_h_bench_mi355x.jsonl]
        leg "chain": CelebA-HQ DDPM-256 mid and SD-v1.5 mid, fp32 and bf16, n chains x `steps` outer steps x `iters` inner iterations: the one chain
        call against the Python composition it replaces -- eng.primal / eng.jvp / eng.vjp with torch for the residual, the recurrence and the
        update -- median of `reps` device-synchronised calls after a warm-up, with the launches of the chain call (dpb_engine_stats).
        leg "drift": at full size and EQUAL h_shift, the off-axis distance h_off of newton_h_chain beside inv_jac_chain's: the gradient chain's step
        size is bisected until its final h_shift matches the Newton chain's (both signs folded: |h_shift|).
    rocprofv3 --kernel-trace --stats -d DIR -o t --output-format csv -- python tools/gpu_newton_h_bench.py --leg traced [--n 4] [--dtype fp32] [--net ddpm]
        runs `--calls` chain calls and nothing else, for the trace.
    python tools/gpu_newton_h_bench.py --leg split --trace-dir DIR [--out FILE.jsonl]
        reads DIR/**/*kernel_trace.csv: the share of the device time spent in the kernels of csrc/cgls.hip (cgls_* and newton_*).
It makes no claim beyond these numbers.  No existing kernel or build line changed with the chain, so there is no headline A/B to run."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T, DAMPING, FRAC = 600.0, 0.1, 0.25


def _net(kind, dtype, n):
    import torch
    from diffusion_pullback_amd import PullbackUNet, configs as cf
    if kind == "ddpm":
        params = cf.ddpm_init_params(cf.CELEBA_HQ_256, seed=0, spectrum=cf.Spectrum())
        net = PullbackUNet("ddpm", cf.CELEBA_HQ_256, params, dtype=dtype, device="cuda:0", max_batch=n, max_rank=max(n, 2), upto=("mid", 0), verbose=False)
        ctx = None
    else:
        cfg = cf.sd_config_for("runwayml/stable-diffusion-v1-5")
        net = PullbackUNet("sd", cfg, cf.sd_init_params(cfg, seed=0), dtype=dtype, device="cuda:0", max_batch=n, max_rank=max(n, 2), upto=("mid", 0),
                           verbose=False)
        ctx = torch.randn(n, cfg.ctx_len, cfg.cross_dim, generator=torch.Generator().manual_seed(1)).cuda()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(n, *net.in_shape, generator=g).cuda()
    u = torch.randn(net.engine.tap_numel(("mid", 0)), 2, generator=g).cuda()
    h0 = net.get_h(x[:1], T, None if ctx is None else ctx[:1], op="mid", block_idx=0)
    scale = FRAC * float(h0.float().norm()) / float(u[:, 0].norm())
    return net, x, u, ctx, scale


def _rows(n):
    return [b % 2 for b in range(n)], [1.0 - 2.0 * (b // 2 % 2) for b in range(n)]


def _chain(net, x, u, ctx, scale, steps, iters, final_shift=True):
    dirs, signs = _rows(x.shape[0])
    return net.newton_h_chain(x=x, t=T, u=u, dirs=dirs, signs=signs, scale=scale, steps=steps, iters=iters, damping=DAMPING, tol=0.0,
                              encoder_hidden_states=ctx, op="mid", block_idx=0, check=False, final_shift=final_shift)


def _composed(net, x, u, ctx, scale, steps, iters):
    """what the chain call replaces: the engine's passes from Python, torch for everything between them (fp32 vectors, fp64 scalars)"""
    import torch
    eng, tap = net.engine, ("mid", 0)
    dirs, signs = _rows(x.shape[0])
    c = torch.stack([signs[b] * u[:, dirs[b]] for b in range(x.shape[0])]).float()
    cur, h0 = x, None
    for j in range(steps):
        eng.primal(cur, T, ctx, tap)
        h = eng.read(tap).reshape(x.shape[0], -1)
        h0 = h if h0 is None else h0
        r = h0 + ((j + 1) / steps) * scale * c - h
        s = eng.vjp(tap, r)
        p, delta = s.clone(), torch.zeros_like(s)
        gamma = (s.double() ** 2).sum(1)
        mu = DAMPING * gamma / (r.double() ** 2).sum(1)
        for _ in range(iters):
            q = eng.jvp(tap, p)
            alpha = gamma / ((q.double() ** 2).sum(1) + mu * (p.double() ** 2).sum(1))
            delta = delta + alpha[:, None].float() * p
            r = r - alpha[:, None].float() * q
            s = eng.vjp(tap, r) - mu[:, None].float() * delta
            g1 = (s.double() ** 2).sum(1)
            p = s + (g1 / gamma)[:, None].float() * p
            gamma = g1
        cur = cur + delta.reshape(x.shape)
    return cur


def _timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ms), 3), [round(v, 3) for v in ms]


def leg_chain(a, rows):
    import torch
    for kind in a.nets:
        for dtype in (torch.float32, torch.bfloat16):
            for n in a.n:
                net, x, u, ctx, scale = _net(kind, dtype, n)
                chain_ms, chain_all = _timed(lambda: _chain(net, x, u, ctx, scale, a.steps, a.iters), a.reps)
                launches = net.engine.stats()[0]
                comp_ms, comp_all = _timed(lambda: _composed(net, x, u, ctx, scale, a.steps, a.iters), a.reps)
                r = _chain(net, x, u, ctx, scale, a.steps, a.iters)
                ref = _composed(net, x, u, ctx, scale, a.steps, a.iters)
                rows.append(dict(leg="chain", net=f"{kind}_mid", dtype=str(dtype).split(".")[-1], chains=n, steps=a.steps, iters=a.iters, chain_ms=chain_ms,
                                 composed_ms=comp_ms, composed_over_chain=round(comp_ms / chain_ms, 3), chain_ms_all=chain_all, composed_ms_all=comp_all,
                                 chain_launches=launches, chain_ms_per_chain_step=round(chain_ms / (n * a.steps), 3),
                                 states_rel_diff=float((r["states"][:, -1] - ref).norm() / ref.norm()),
                                 h_shift_over_asked=[round(float(v) / (scale * float(u[:, 0].norm())), 4) for v in r["h_shift"][:, -1]]))
                print(json.dumps(rows[-1]), flush=True)
                del net
                torch.cuda.empty_cache()


def leg_drift(a, rows):
    import torch
    for kind in a.nets:
        n = 4
        net, x, u, ctx, scale = _net(kind, torch.float32, n)
        dirs, signs = _rows(n)
        r = _chain(net, x, u, ctx, scale, a.steps, a.iters)
        want = r["h_shift"][:, -1].abs()
        lo, hi = torch.zeros(n), torch.full((n,), 64.0)
        for _ in range(12):                                   # bisect every chain's step size on |h_shift| at the last state
            mid = (lo + hi) / 2
            g = net.inv_jac_chain(x=x, t=T, u=u, dirs=dirs, signs=signs, steps=2 * a.steps, step_size=mid.tolist(), encoder_hidden_states=ctx, op="mid",
                                  block_idx=0, check=False)
            over = g["h_shift"][:, -1].abs().cpu() > want.cpu()
            hi = torch.where(over, mid, hi); lo = torch.where(over, lo, mid)
        off_g = (g["h_dist"][:, -1] ** 2 - g["h_shift"][:, -1] ** 2).clamp(min=0).sqrt()
        rows.append(dict(leg="drift", net=f"{kind}_mid", dtype="float32", chains=n, newton_steps=a.steps, newton_iters=a.iters, gradient_steps=2 * a.steps,
                         h_shift_newton=[float(v) for v in r["h_shift"][:, -1]], h_shift_gradient=[float(v) for v in g["h_shift"][:, -1]],
                         h_off_over_shift_newton=[round(float(v), 4) for v in r["h_off"][:, -1] / want],
                         h_off_over_shift_gradient=[round(float(v), 4) for v in off_g / g["h_shift"][:, -1].abs()], gradient_step_size=mid.tolist()))
        print(json.dumps(rows[-1]), flush=True)
        del net
        torch.cuda.empty_cache()


def leg_traced(a):
    import torch
    dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[a.dtype]
    net, x, u, ctx, scale = _net(a.nets[0], dtype, a.n[0])
    for _ in range(a.calls):
        _chain(net, x, u, ctx, scale, a.steps, a.iters)
        torch.cuda.synchronize()


def leg_split(a, rows):
    hits = sorted(glob.glob(os.path.join(a.trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    if not hits:
        raise SystemExit(f"no *kernel_trace.csv under {a.trace_dir}")
    us, cnt = {}, {}
    with open(hits[0]) as fh:
        for r in csv.DictReader(fh):
            name = r["Kernel_Name"]
            key = "solver" if "cgls_" in name else "newton" if "newton_" in name else "chain_shift" if "chain_shift_kernel" in name else "passes"
            us[key] = us.get(key, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            cnt[key] = cnt.get(key, 0) + 1
    tot = sum(us.values())
    rows.append(dict(leg="split", device_us={k: round(v, 1) for k, v in us.items()}, launches=cnt,
                     new_kernels_share=round((us.get("solver", 0) + us.get("newton", 0)) / tot, 5)))
    print(json.dumps(rows[-1]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default="chain,drift")
    ap.add_argument("--nets", type=lambda s: s.split(","), default=["ddpm", "sd"])
    ap.add_argument("--n", type=lambda s: [int(v) for v in s.split(",")], default=[1, 4, 8])
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--trace-dir", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = []
    for leg in a.leg.split(","):
        if leg == "chain":
            leg_chain(a, rows)
        elif leg == "drift":
            leg_drift(a, rows)
        elif leg == "traced":
            leg_traced(a)
        elif leg == "split":
            leg_split(a, rows)
        else:
            raise SystemExit(f"unknown leg {leg!r}")
    if a.out and rows:
        with open(a.out, "a") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
