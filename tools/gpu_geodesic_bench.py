"""Not a test: records what the pullback-geodesic chain (PullbackUNet.pullback_geodesic, dpb_geodesic_chain) costs on ONE MI355X in ONE session, and what
it finds at full size.
    python tools/gpu_geodesic_bench.py [--nets ddpm256,sd15] [--m 4,8,16] [--iters 4] [--reps 5] [--out profiles/geodesic_bench_mi355x.jsonl]
        leg "chain": CelebA-HQ DDPM-256 and SD-v1.5 (synthetic weights, the tape up to the mid tap), fp32 and bf16, a slerp curve of m interior points:
        ONE chain call of `iters` iterations with the final energy against the Python composition it replaces -- per iteration get_h on the whole
        curve, the cotangents and the energy in torch, eng.primal + eng.vjp on the interior rows, the torch update, the energy read on the host --
        median of `reps` device-synchronised calls after a warm-up, with the launches of the chain call (dpb_engine_stats).
        leg "quality": fp32, m = --quality-m, a FIXED 40 iterations (tol 0, check_every 4, the step rule's eta and the driver's halving): energy,
        h-length and uniformity of the lerp, the slerp and the geodesic curve by curve_energy, and the driver's record.
It makes no claim beyond these numbers.  No existing kernel or build line changed with the chain, so there is no headline A/B to run."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T = 600.0
TAP = ("mid", 0)


def _net(name, dtype, m):
    import torch
    from diffusion_pullback_amd import PullbackUNet, configs as cf
    from diffusion_pullback_amd.pullback import geodesic_init
    g = torch.Generator().manual_seed(0)
    if name == "ddpm256":
        params = cf.ddpm_init_params(cf.CELEBA_HQ_256, seed=0, spectrum=cf.Spectrum())
        net = PullbackUNet("ddpm", cf.CELEBA_HQ_256, params, dtype=dtype, device="cuda:0", max_batch=m + 2, max_rank=max(m, 2), upto=TAP, verbose=False)
        ctx = None
    else:
        cfg = cf.sd_config_for("runwayml/stable-diffusion-v1-5")
        net = PullbackUNet("sd", cfg, cf.sd_init_params(cfg, seed=0), dtype=dtype, device="cuda:0", max_batch=m + 2, max_rank=max(m, 2), upto=TAP, verbose=False)
        ctx = torch.randn(1, cfg.ctx_len, cfg.cross_dim, generator=g).cuda()
    xa, xb = torch.randn(*net.in_shape, generator=g), torch.randn(*net.in_shape, generator=g)
    return net, geodesic_init(xa, xb, m, "slerp").cuda(), ctx


def _chain(net, P, ctx, eta, iters):
    return net.engine.geodesic_chain(P, T, ctx, TAP, eta, 0.0, iters, True)


def _composed(net, P, ctx, eta, iters):
    """what the chain call replaces: Python between the passes, one energy read per iteration"""
    import torch
    eng, cur, energy = net.engine, P, []
    cm = None if ctx is None else ctx.expand(P.shape[0] - 2, -1, -1)
    for _ in range(iters):
        h = net.get_h(cur, T, None if ctx is None else ctx.expand(P.shape[0], -1, -1), op=TAP[0], block_idx=TAP[1]).flatten(1).double()
        energy.append(float(0.5 * ((h[1:] - h[:-1]) ** 2).sum()))                  # the host reads the energy: a synchronisation per iteration
        cot = (2 * h[1:-1] - h[:-2] - h[2:]).float()
        eng.primal(cur[1:-1], T, cm, TAP)
        W = eng.vjp(TAP, cot)
        nxt = cur.clone()
        nxt[1:-1] = (cur[1:-1].double() - eta * W.view_as(cur[1:-1]).double()).float()
        cur = nxt
    h = net.get_h(cur, T, None if ctx is None else ctx.expand(P.shape[0], -1, -1), op=TAP[0], block_idx=TAP[1]).flatten(1).double()
    energy.append(float(0.5 * ((h[1:] - h[:-1]) ** 2).sum()))
    return cur, energy


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


def _eta(net, P, ctx):
    _, _, _, st, csq = net.engine.geodesic_chain(P, T, ctx, TAP, 0.0, 0.0, 1, False)
    return 0.25 * float(csq[0].sum()) / float(st[0, :, 1].sum())


def _emit(a, row):
    """printed, and appended to --out at once: a later configuration that fails loses nothing"""
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(json.dumps(row) + "\n")


def leg_chain(a):
    import torch
    for name in a.nets:
        for dtype in (torch.float32, torch.bfloat16):
            for m in a.m:
                net, P, ctx = _net(name, dtype, m)
                eta = _eta(net, P, ctx)
                chain_ms, chain_all = _timed(lambda: _chain(net, P, ctx, eta, a.iters), a.reps)
                launches = net.engine.stats()[0]
                comp_ms, comp_all = _timed(lambda: _composed(net, P, ctx, eta, a.iters), a.reps)
                curves, seg_h = _chain(net, P, ctx, eta, a.iters)[:2]
                ref, energy = _composed(net, P, ctx, eta, a.iters)
                _emit(a, dict(leg="chain", net=f"{name}_mid", dtype=str(dtype).split(".")[-1], m=m, iters=a.iters, eta=eta, chain_ms=chain_ms,
                                 composed_ms=comp_ms, composed_over_chain=round(comp_ms / chain_ms, 3), chain_ms_all=chain_all, composed_ms_all=comp_all,
                                 chain_launches=launches, chain_ms_per_iteration=round(chain_ms / a.iters, 3),
                                 curve_rel_diff=float((curves[-1] - ref).norm() / ref.norm()), energy_chain=[0.5 * float(s.sum()) for s in seg_h],
                              energy_composed=energy))
                del net
                torch.cuda.empty_cache()


def leg_quality(a):
    import torch
    from diffusion_pullback_amd.pullback import geodesic_init
    for name in a.nets:
        m = a.quality_m
        net, P, ctx = _net(name, torch.float32, m)
        t0 = time.perf_counter()
        geo, info = net.pullback_geodesic(P[:1], P[-1:], T, n_points=m, op=TAP[0], block_idx=TAP[1], encoder_hidden_states=ctx, init="slerp", max_iter=40,
                                          tol=0.0, check_every=4)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        curves = {"lerp": geodesic_init(P[0], P[-1], m, "linear"), "slerp": P, "geodesic": geo}
        stats = {k: net.curve_energy(c, T, op=TAP[0], block_idx=TAP[1], encoder_hidden_states=ctx) for k, c in curves.items()}
        _emit(a, dict(leg="quality", net=f"{name}_mid", dtype="float32", m=m, max_iter=40, wall_s=round(wall, 3),
                         **{f"{k}_{q}": stats[k][q] for k in stats for q in ("energy", "length_h", "length_x", "uniformity")},
                         energy_by_block=info["energy"], decisions=info["decisions"], halvings=info["halvings"], iterations=info["iterations"],
                      attempted=info["attempted"], rises=info["rises"], step_size=info["step_size"]))
        del net
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default="chain,quality")
    ap.add_argument("--nets", type=lambda s: s.split(","), default=["ddpm256", "sd15"])
    ap.add_argument("--m", type=lambda s: [int(v) for v in s.split(",")], default=[4, 8, 16])
    ap.add_argument("--quality-m", type=int, default=8)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    for leg in a.leg.split(","):
        if leg == "chain":
            leg_chain(a)
        elif leg == "quality":
            leg_quality(a)
        else:
            raise SystemExit(f"unknown leg {leg!r}")


if __name__ == "__main__":
    main()
