"""Not a test: times the sampling of local tangent spaces over a grid of (sample, t) pairs -- SD-1.5, mid tap, bf16 -- two ways on ONE full-size
engine, in one session:
  (a) batch        PullbackUNet.local_encoder_pullback_batch: the pairs of a group advance together, each at its own timestep (dpb_primal_t, then
                   one dpb_pullback_iterate pass of all their directions per iteration);
  (b) one_by_one   local_encoder_pullback_zt per pair: what run_sample_encoder_local_tangent_space_zt of the reference does.
    python tools/gpu_tspace_bench.py [--dtype bf16] [--samples 2] [--times 0.8,0.5] [--ranks 10,50] [--tangents 100] [--iters 12] [--reps 3] [--out FILE.jsonl]
Both legs run exactly `iters` iterations per pair (min_iter = max_iter = iters: the stop rule cannot fire), so the legs do the same work.  Per rank
k the pairs go through in groups of min(pairs, tangents // k).  Prints (and writes to --out) per leg and rank: seconds per grid (median of `reps`
device-synchronised runs, the legs alternated), pairs/s, and the summary ratio (a)/(b); before timing, the two legs' singular values are compared."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from diffusion_pullback_amd import PullbackUNet, configs as cf  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--samples", type=int, default=2)
    ap.add_argument("--times", default="0.8,0.5")
    ap.add_argument("--ranks", default="10,50")
    ap.add_argument("--tangents", type=int, default=100)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    ranks = [int(k) for k in a.ranks.split(",")]
    times = [1000.0 * float(v) - 1.0 for v in a.times.split(",")]              # timesteps of the h_t values
    pairs = [(i, t) for t in times for i in range(a.samples)]
    group = {k: max(1, min(len(pairs), a.tangents // k)) for k in ranks}
    g = torch.Generator().manual_seed(0)
    net = PullbackUNet("sd", cf.SD15, cf.sd_init_params(cf.SD15, seed=0, spectrum=cf.Spectrum()), dtype=dtype, device="cuda:0",
                       max_batch=max(group.values()), max_rank=max(group[k] * k for k in ranks), upto=("mid", 0), verbose=False)
    xs = torch.randn(a.samples, 4, 64, 64, generator=g).cuda()
    ctx = torch.randn(1, 77, 768, generator=g).cuda()
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    emit(dict(model="sd15", dtype=a.dtype, tap="mid", pairs=len(pairs), samples=a.samples, timesteps=times, iters=a.iters, reps=a.reps, groups=group,
              device=torch.cuda.get_device_name(0)))
    for k in ranks:
        V0 = torch.linalg.qr(torch.randn(net.engine.n_in, k, generator=g))[0].T.contiguous().cuda()
        kw = dict(op="mid", block_idx=0, pca_rank=k, min_iter=a.iters, max_iter=a.iters, convergence_threshold=1e-3, V0=V0)

        def batch():
            out = []
            for g0 in range(0, len(pairs), group[k]):
                part = pairs[g0:g0 + group[k]]
                _, s, _, _ = net.local_encoder_pullback_batch(xs[[i for i, _ in part]], torch.tensor([t for _, t in part]), ctx, **kw)
                out.append(s)
            return torch.cat(out)

        def one_by_one():
            return torch.stack([net.local_encoder_pullback_zt(xs[i:i + 1], t, ctx, chunk_size=k, **kw)[1] for i, t in pairs])

        sa, sb = batch(), one_by_one()                     # warm-up of both legs, and the check that they sample the same spaces
        emit(dict(check="same singular values", k=k, max_rel=float(((sa - sb).abs() / sb.abs()).max())))
        sec = {"batch": [], "one_by_one": []}
        for _ in range(a.reps):                            # alternate the legs
            for name, fn in (("batch", batch), ("one_by_one", one_by_one)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                sec[name].append(time.perf_counter() - t0)
        ma, mb = statistics.median(sec["batch"]), statistics.median(sec["one_by_one"])
        for name, m in (("batch", ma), ("one_by_one", mb)):
            emit(dict(leg=name, k=k, group=group[k] if name == "batch" else 1, s_per_grid=round(m, 4), pairs_per_s=round(len(pairs) / m, 3),
                      runs_s=[round(v, 4) for v in sec[name]]))
        emit(dict(summary=f"sd15 mid {a.dtype} k={k}", batch_s=round(ma, 4), one_by_one_s=round(mb, 4), batch_over_one_by_one_time=round(ma / mb, 3)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.writelines(json.dumps(d) + "\n" for d in lines)


if __name__ == "__main__":
    main()
