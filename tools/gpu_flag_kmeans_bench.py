"""Not a test: times flag k-means (geometry.flag_kmeans, dpb_flag_kmeans_*) and the chordal affinity (geometry.flag_affinity) on the project's standard
size -- B = 100 local bases of k = 50 rows -- planted as C = 4 families of 25 with r = 10 shared directions each and 40 private rows, Gaussian, shuffled.
    python tools/gpu_flag_kmeans_bench.py [--n 16384,32768,81920,196608] [--reps 5] [--out FILE.jsonl]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/gpu_flag_kmeans_bench.py --leg trace --n-one 16384
Every size runs in a fresh child process under its own time limit (--leg-timeout seconds); the first that fails or runs out of time ends the run.  One
JSON line per N, appended to --out as well; every time is the median of --reps after a warm-up, all in one session:
  total_ms              geometry.flag_kmeans from the default seeding to the centres, its host reads included
  init_ms, update_ms, assign_ms, finish_ms   from a run with timings=True (a device synchronisation at each boundary): the cross-Gram pass, the whitening
                        and the seeding; per fit the gathers and the flag-mean solves of the changed clusters, and the assignment pass with its host
                        read (lists, one entry per fit, of the last timed run); the coefficient pass over X
  rounds, moved, inner_iterations, recovered   of that run; recovered: the planted partition
  inside_*              the same from a hard start, every seed inside planted family 0: rounds with moves, and their update and assignment times
  torch_fp64_ms         the same run through the float64 torch composition on the same GPU: batched qr once, then per round per cluster the Gram of
                        the stacked Q's, eigh, the top r rows, ||Q Y^T||_F^2 (same seeds, same move rule); labels_equal and the largest principal
                        angle between the two sets of centres (angle_to_torch, rad)
  affinity_ms           geometry.flag_affinity of the 100 members against the 4 centres; affinity_torch_ms: qr of both stacks and ||Q_a Q_y^T||_F^2 in
                        float64 torch; affinity_err_to_torch
The trace leg runs one flag k-means, one flag mean of the same set (r = 10: fm_product_kernel at m = 32 on the same Ghat) and a device copy of the
bytes of Ghat, for a kernel trace taken around it."""
import argparse
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
    return statistics.median(ts) * 1e3, [round(x * 1e3, 3) for x in ts]


def _set(b, k, n, c, r, seed):
    """(x [B, k, N] fp32, truth [B]): family f's members share r Gaussian rows, perturbed per member by 0.3 N(0, 1); the rest are their own"""
    import torch
    g = torch.Generator(device=DEV).manual_seed(seed)
    shared = torch.randn(c, r, n, generator=g, device=DEV)
    x = torch.randn(b, k, n, generator=g, device=DEV)
    truth = torch.arange(b, device=DEV) % c
    truth = truth[torch.randperm(b, generator=g, device=DEV)]
    x[:, :r] = shared[truth] + 0.3 * x[:, :r]
    return x, truth


def _same_partition(a, b):
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def _angle(torch, ya, yb):
    qa = torch.linalg.qr(ya.double().T).Q
    qb = torch.linalg.qr(yb.double().T).Q
    return float(torch.asin(torch.linalg.svdvals(qa - qb @ (qb.T @ qa)).max().clamp(max=1.0)))


def _torch_kmeans(torch, q, start, c, r, max_rounds=50):
    """the float64 torch composition: q [B, k, N] orthonormal rows; the same rounds as geometry.flag_kmeans from the same start labels"""
    b = q.shape[0]
    labels = start.clone()
    rounds = 0
    while True:
        ys = []
        for j in range(c):
            qs = q[labels == j].reshape(-1, q.shape[2])
            lam, v = torch.linalg.eigh(qs @ qs.T)
            ys.append((v[:, -r:].flip(1) / lam[-r:].flip(0).sqrt()).T @ qs)
        y = torch.stack(ys)
        aff = torch.einsum("bkn,crn->bckr", q, y).pow(2).sum(dim=(2, 3))
        if rounds == max_rounds:
            break
        own = aff[torch.arange(b), labels]
        best = aff.argmax(dim=1)
        want = torch.where(aff[torch.arange(b), best] > own + 1e-12 * r, best, labels)
        rounds += 1
        if bool((want == labels).all()):
            break
        labels = want
    return labels, y, aff, rounds


def _size_leg(a):
    import torch
    from diffusion_pullback_amd import geometry
    b, k, n, c, r = a.b, a.k, a.n_one, a.c, a.r
    x, truth = _set(b, k, n, c, r, a.seed)
    rec = dict(leg="size", B=b, k=k, N=n, C=c, r=r, R=b * k, seed=a.seed, ghat_gbytes=round(8.0 * (b * k) ** 2 / 1e9, 3))
    run = lambda: geometry.flag_kmeans(x, c, rank=r)
    dt, runs = _timed(run, a.reps)
    rec.update(total_ms=round(dt, 2), total_ms_runs=runs)
    labels, Y, info = geometry.flag_kmeans(x, c, rank=r, timings=True)
    t = info["timings"]
    rec.update(init_ms=round(t["init_ms"], 2), update_ms=[round(v, 2) for v in t["update_ms"]], assign_ms=[round(v, 2) for v in t["assign_ms"]],
               finish_ms=round(t["finish_ms"], 2), rounds=info["rounds"], moved=info["moved"], converged=info["converged"],
               inner_iterations=info["inner_iterations"], inner_converged=info["inner_converged"], sizes=info["sizes"].tolist(),
               objective=[round(float(v), 6) for v in info["objective"]], gap=info["gap"], recovered=_same_partition(labels, truth))
    start = torch.from_numpy(info["start"]).to(DEV).long()          # the comparison starts from the same labels
    # the hard start: every seed inside planted family 0, so that rounds with moves are needed
    inside = (truth == 0).nonzero().flatten()[:c].tolist()
    hl, hy, hi = geometry.flag_kmeans(x, c, rank=r, init=inside, timings=True)
    ht = hi["timings"]
    rec.update(inside_rounds=hi["rounds"], inside_moved=hi["moved"], inside_kept=hi["kept"], inside_converged=hi["converged"],
               inside_recovered=_same_partition(hl, truth), inside_update_ms=[round(v, 2) for v in ht["update_ms"]],
               inside_assign_ms=[round(v, 2) for v in ht["assign_ms"]], inside_objective=[round(float(v), 4) for v in hi["objective"]],
               inside_monotone=hi["monotone"])
    def torch_run():
        q = torch.linalg.qr(x.double().transpose(1, 2)).Q.transpose(1, 2)
        return _torch_kmeans(torch, q, start, c, r)
    dt, runs = _timed(torch_run, max(1, a.reps // 2))
    tl, ty, taff, trounds = torch_run()
    match = _same_partition(labels, tl)
    ang = None
    if match:
        order = [int(tl[(labels == j).nonzero()[0, 0]]) for j in range(c)]
        ang = max(_angle(torch, Y[j], ty[order[j]]) for j in range(c))
    rec.update(torch_fp64_ms=round(dt, 1), torch_fp64_ms_runs=runs, torch_rounds=trounds, labels_equal=match, angle_to_torch=ang)
    dt, runs = _timed(lambda: geometry.flag_affinity(x, Y, check=False), a.reps)
    aff = geometry.flag_affinity(x, Y, check=False)

    def torch_aff():
        qa = torch.linalg.qr(x.double().transpose(1, 2)).Q.transpose(1, 2)
        qy = torch.linalg.qr(Y.double().transpose(1, 2)).Q.transpose(1, 2)
        return torch.einsum("bkn,crn->bckr", qa, qy).pow(2).sum(dim=(2, 3))
    dt2, runs2 = _timed(torch_aff, max(1, a.reps // 2))
    rec.update(affinity_ms=round(dt, 3), affinity_ms_runs=runs, affinity_torch_ms=round(dt2, 1), affinity_err_to_torch=float((aff - torch_aff()).abs().max()),
               affinity_err_to_run=float((aff - info["affinity"]).abs().max()))
    print(json.dumps(rec), flush=True)


def _trace_leg(a):
    import torch
    from diffusion_pullback_amd import geometry
    b, k, n, c, r = a.b, a.k, a.n_one, a.c, a.r
    x, _ = _set(b, k, n, c, r, a.seed)
    geometry.flag_kmeans(x, c, rank=r)
    geometry.flag_mean(x, rank=r, max_iter=16)
    src = torch.empty((b * k) ** 2, dtype=torch.float64, device=DEV)
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    torch.cuda.synchronize()
    print(json.dumps(dict(leg="trace", B=b, k=k, N=n, C=c, r=r, ghat_bytes=8 * (b * k) ** 2)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="16384,32768,81920,196608")
    ap.add_argument("--b", type=int, default=100)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--c", type=int, default=4)
    ap.add_argument("--r", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=97)
    ap.add_argument("--leg-timeout", type=int, default=240)
    ap.add_argument("--out", default="")
    ap.add_argument("--leg", default="", help="trace: one run of each kernel family, for a kernel trace taken around this process")
    ap.add_argument("--n-one", type=int, default=16384, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg == "trace":
        return _trace_leg(a)
    if a.leg:
        return _size_leg(a)
    for n in a.n.split(","):
        cmd = ["timeout", "-k", "10", str(a.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", "size", "--n-one", n, "--b", str(a.b),
               "--k", str(a.k), "--c", str(a.c), "--r", str(a.r), "--reps", str(a.reps), "--seed", str(a.seed)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        for ln in lines:
            print(ln, flush=True)
            if a.out:
                with open(a.out, "a") as fh:
                    fh.write(ln + "\n")
        if r.returncode != 0 or not lines:                     # a fault, an abort or a time limit: nothing more is started on the GPU
            print(json.dumps(dict(leg="size", N=int(n), failed=True, returncode=r.returncode, stderr=r.stderr[-800:])), flush=True)
            sys.exit(1)


if __name__ == "__main__":
    main()
