"""Not a test: times an h-space traversal of ONE sample -- 5 directions x 5 scales at the mid tap of SD-1.5, bf16, in calls of max_batch rows --
three ways on ONE full-size engine:
  (a) shared_prefix   PullbackUNet.h_traversal: dpb_forward_shift with x [1], the net up to the tap once per call;
  (b) repeated_x      dpb_forward_shift with x repeated to the rows of the call (one ordinary forward pass per call);
  (c) composition     what the library offered before: get_h once, then get_h_to_e(x repeated, h + s u) per call.
    python tools/gpu_hshift_bench.py [--dtype bf16] [--max-batch 5] [--dirs 5] [--scales 5] [--iters 4] [--reps 7] [--out FILE.jsonl]
Prints (and appends to --out) per leg: traversals/s and ms per traversal (median of `reps` windows of `iters` traversals each, device-synchronised,
the legs alternated), the dpb_engine_stats of the last call (launches, algorithmic GEMM flops), and the summary ratios (a)/(c), (a)/(b) of the
times with the flop share of the part of the net after the tap next to them."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from diffusion_pullback_amd import PullbackUNet, configs as cf  # noqa: E402


def timed(fn, iters, reps):
    fn()                                                  # warm-up: code objects, GEMM plans of both batch sizes
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / iters * 1e3)
    return statistics.median(ms), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--max-batch", type=int, default=5)
    ap.add_argument("--dirs", type=int, default=5)
    ap.add_argument("--scales", type=int, default=5)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    g = torch.Generator().manual_seed(0)
    net = PullbackUNet("sd", cf.SD15, cf.sd_init_params(cf.SD15, seed=0, spectrum=cf.Spectrum()), dtype=dtype, device="cuda:0", max_batch=a.max_batch,
                       max_rank=1, verbose=False)
    x, t, ctx = torch.randn(1, 4, 64, 64, generator=g).cuda(), 696.2727, torch.randn(1, 77, 768, generator=g).cuda()
    e = net.engine
    tap, mb = ("mid", 0), a.max_batch
    n_h = e.tap_numel(tap)
    u = torch.linalg.qr(torch.randn(n_h, a.dirs, generator=g))[0].cuda()                       # [D, k], as the pullbacks return it
    scales = [float(s) for s in torch.linspace(-2.0, 2.0, a.scales)]
    rows = [(i, s) for i in range(a.dirs) for s in scales]
    chunks = [rows[i:i + mb] for i in range(0, len(rows), mb)]
    UT = (u / u.norm(dim=0, keepdim=True)).T.contiguous()
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    def shared():
        return net.h_traversal(x, t, ctx, u, scales, "mid", 0)

    def repeated():
        return torch.cat([e.forward_shift(x.expand(len(c), -1, -1, -1), t, ctx, tap, UT, [r[0] for r in c], [r[1] for r in c]) for c in chunks])

    def composition():
        h = net.get_h(x, t, ctx, "mid", 0)
        out = []
        for c in chunks:
            hs = torch.cat([h + s * UT[i].reshape(h.shape) for i, s in c])
            out.append(net.get_h_to_e(x, t, ctx, hs, "mid", 0))
        return torch.cat(out)

    # flop shares from the engine's own counters: the whole net and the part up to the tap, at the call's batch
    e.forward(x.expand(mb, -1, -1, -1), t, ctx, "eps"); f_eps = e.stats()[1]
    e.forward(x.expand(mb, -1, -1, -1), t, ctx, tap); f_tap = e.stats()[1]
    e.forward(x, t, ctx, tap); f_tap1 = e.stats()[1]
    emit(dict(model="sd15", dtype=a.dtype, tap="mid", rows=len(rows), max_batch=mb, calls=len(chunks), iters=a.iters, reps=a.reps,
              device=torch.cuda.get_device_name(0), gemm_gflop_full_call=round(f_eps / 1e9, 1),
              flop_share_after_tap=round((f_eps - f_tap) / f_eps, 4), flop_share_shared_prefix_call=round((f_tap1 + f_eps - f_tap) / f_eps, 4)))
    ra, rb, rc = shared().reshape(len(rows), -1), repeated().reshape(len(rows), -1), composition().reshape(len(rows), -1)
    rel = lambda p, q: float((p - q).norm() / q.norm())
    emit(dict(check="same results", rel_shared_vs_repeated=rel(ra, rb), rel_shared_vs_composition=rel(ra, rc)))
    med = {}
    for _ in range(2):                                    # alternate the legs
        for name, fn in (("shared_prefix", shared), ("repeated_x", repeated), ("composition", composition)):
            m, ms = timed(fn, a.iters, a.reps)
            launches, flops, _ = e.stats()
            med.setdefault(name, []).append(m)
            emit(dict(leg=name, ms_per_traversal=round(m, 3), traversals_per_s=round(1e3 / m, 2), windows_ms=[round(v, 3) for v in ms],
                      last_call_launches=launches, last_call_gemm_gflop=round(flops / 1e9, 1)))
    ma, mb_, mc = (statistics.median(med[k]) for k in ("shared_prefix", "repeated_x", "composition"))
    emit(dict(summary="sd15 mid " + a.dtype, shared_prefix_ms=round(ma, 3), repeated_x_ms=round(mb_, 3), composition_ms=round(mc, 3),
              shared_over_composition_time=round(ma / mc, 3), shared_over_repeated_time=round(ma / mb_, 3)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.writelines(json.dumps(d) + "\n" for d in lines)


if __name__ == "__main__":
    main()
