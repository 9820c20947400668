"""Not a test: records what the parallel-h chain (PullbackUNet.inv_jac_chain, dpb_inv_jac_chain) costs on ONE MI355X in ONE session.
    python tools/gpu_parallel_h_bench.py [--n 1,4,8] [--steps 4] [--reps 5] [--out profiles/parallel_h_bench_mi355x.jsonl]
        leg "chain": CelebA-HQ DDPM-256, mid tap, fp32 and bf16, n chains x `steps` steps with the SEGA rule on: the one chain call against the Python
        composition it replaces -- inv_jac_xt per chain and step, then torch std / mask / add -- median of `reps` device-synchronised calls after a
        warm-up, with the launches of the chain call (dpb_engine_stats).
        leg "job": run_edit_global_frechet_mean_zt (space h, --edit_xt parallel-h, --local_projection False, bases cached by a first call without
        chains) at trajectory_batch 1 against the default, fp32, wall clock of the whole call.
    rocprofv3 --kernel-trace --hip-trace --stats -d DIR -o t --output-format csv -- python tools/gpu_parallel_h_bench.py --leg traced --what chain|composed [--n 4] [--dtype fp32]
        runs `--calls` calls and nothing else, for the trace.
    python tools/gpu_parallel_h_bench.py --leg split --trace-dir DIR --what chain|composed [--n 4] [--calls 3] [--out FILE.jsonl]
        reads DIR/**/t_kernel_trace.csv and t_hip_api_trace.csv: device time per step by phase -- primal (to the tap), adjoint, dpb_direction_step,
        shift statistics -- told apart by the chain's own kernels in launch order, and the hipStreamSynchronize / hipDeviceSynchronize calls per call.
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

SIGMA, STEP = 1.0, 2.0


def _net(dtype, n):
    import torch
    from diffusion_pullback_amd import PullbackUNet, configs as cf
    params = cf.ddpm_init_params(cf.CELEBA_HQ_256, seed=0, spectrum=cf.Spectrum())
    net = PullbackUNet("ddpm", cf.CELEBA_HQ_256, params, dtype=dtype, device="cuda:0", max_batch=n, max_rank=max(n, 2), upto=("mid", 0), verbose=False)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(n, *net.in_shape, generator=g).cuda()
    u = torch.randn(net.engine.tap_numel(("mid", 0)), 2, generator=g).cuda()
    return net, x, u


def _chain(net, x, u, steps, final_shift=True):
    n = x.shape[0]
    return net.inv_jac_chain(x=x, t=600.0, u=u, dirs=[b % 2 for b in range(n)], signs=[1.0 - 2.0 * (b // 2 % 2) for b in range(n)], steps=steps,
                             step_size=STEP, sega_sigma=SIGMA, op="mid", block_idx=0, check=False, final_shift=final_shift)


def _composed(net, x, u, steps):
    """what the chain call replaces, chain after chain: inv_jac_xt at the current state, the SEGA mask from torch's std, the step"""
    import torch
    out = []
    for b in range(x.shape[0]):
        c = (1.0 - 2.0 * (b // 2 % 2)) * u[:, b % 2]
        states = [x[b:b + 1]]
        for _ in range(steps):
            cur = states[-1]
            v = net.inv_jac_xt(x=cur, t=600.0, op="mid", block_idx=0, u=c)
            v = v.masked_fill(v.abs() < SIGMA * v.std(), 0.0)
            states.append(cur + v.reshape(cur.shape) * STEP)
        out.append(torch.cat(states))
    return torch.stack(out)


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
    for dtype in (torch.float32, torch.bfloat16):
        for n in a.n:
            net, x, u = _net(dtype, n)
            chain_ms, chain_all = _timed(lambda: _chain(net, x, u, a.steps), a.reps)
            launches = net.engine.stats()[0]
            lean_ms, _ = _timed(lambda: _chain(net, x, u, a.steps, final_shift=False), a.reps)     # without the forward pass of the last h_shift
            comp_ms, comp_all = _timed(lambda: _composed(net, x, u, a.steps), a.reps)
            r = _chain(net, x, u, a.steps)
            ref = _composed(net, x, u, a.steps)
            rows.append(dict(leg="chain", net="ddpm256_mid", dtype=str(dtype).split(".")[-1], chains=n, steps=a.steps, sega_sigma=SIGMA, chain_ms=chain_ms,
                             composed_ms=comp_ms, chain_ms_without_final_shift=lean_ms, composed_over_chain=round(comp_ms / chain_ms, 3), chain_ms_all=chain_all, composed_ms_all=comp_all,
                             chain_launches=launches, chain_ms_per_chain_step=round(chain_ms / (n * a.steps), 3),
                             states_rel_diff=float((r["states"] - ref).norm() / ref.norm()), kept_last=[int(v) for v in r["sega_kept"][:, -1].tolist()]))
            print(json.dumps(rows[-1]), flush=True)
            del net
            torch.cuda.empty_cache()


def leg_job(a, rows, tmp):
    import torch
    from diffusion_pullback_amd import main as m
    from diffusion_pullback_amd.edit import EditUncondDiffusion
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        argv = ["--note", "bench", "--model_name", "CelebA_HQ_HF", "--dataset_name", "Random", "--result_folder", os.path.join(tmp, "runs"), "--performance_boosting_t",
                "0.2", "--edit_t", "0.6", "--h_t", "0.8", "--run_edit_global_frechet_mean_zt", "True", "--frechet_mean_space", "h", "--num_local_basis", "2",
                "--pca_rank", "2", "--vis_num_pc", "2", "--vis_num", str(a.steps), "--edit_xt", "parallel-h", "--x_edit_step_size", str(STEP * a.steps),
                "--use_sega_reg", "True", "--local_projection", "False"]
        args = m.preset(m.parse_args(argv))
        ed = EditUncondDiffusion(args, unet=m.build_unet(args))
        kw = dict(idx=0, op="mid", block_idx=0, vis_num=a.steps, pca_rank=2, num_local_basis=2, local_projection=False, frechet_mean_space="h")
        t0 = time.perf_counter()
        ed.run_edit_global_frechet_mean_zt(vis_num_pc=0, **kw)          # no chains: samples the two local bases, computes and caches the global one
        torch.cuda.synchronize()
        prime = time.perf_counter() - t0
        res = {}
        for tb in (ed.trajectory_batch, 1, ed.trajectory_batch, 1):      # (each setting twice: the first pair also loads every code object)
            ed.trajectory_batch = tb
            for f in glob.glob(os.path.join(ed.result_folder, "x0_gen-*.png")):
                os.remove(f)
            t0 = time.perf_counter()
            out = ed.run_edit_global_frechet_mean_zt(vis_num_pc=2, **kw)
            torch.cuda.synchronize()
            res.setdefault(tb, []).append(round(time.perf_counter() - t0, 3))
            assert len(out["names"]) == 4
        tbs = sorted(res)
        rows.append(dict(leg="job", net="ddpm256_mid", dtype="float32", chains=4, steps=a.steps, for_steps=args.for_steps, bases_s=round(prime, 3),
                         job_s_by_trajectory_batch={str(k): v for k, v in res.items()}, one_at_a_time_over_together=round(res[tbs[0]][-1] / res[tbs[-1]][-1], 3)))
        print(json.dumps(rows[-1]), flush=True)
    finally:
        os.chdir(cwd)


def leg_traced(a):
    import torch
    dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[a.dtype]
    net, x, u = _net(dtype, a.n[0])
    for _ in range(a.calls):
        (_chain if a.what == "chain" else _composed)(net, x, u, a.steps)
        torch.cuda.synchronize()


def _find(d, suffix):
    hits = sorted(glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True))
    return hits[0] if hits else None


def leg_split(a, rows):
    kt = _find(a.trace_dir, "kernel_trace.csv")
    if not kt:
        raise SystemExit(f"no *kernel_trace.csv under {a.trace_dir}")
    with open(kt) as fh:
        ks = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    row = dict(leg="split", what=a.what, net="ddpm256_mid", dtype=a.dtype, chains=a.n[0], steps=a.steps, calls=a.calls)
    per = a.calls * a.steps
    if a.what == "chain":
        phase, shifts = "idle", 0
        us, cnt = {}, {}
        for r in ks:
            name, dt = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            if "chain_shift_kernel" in name:
                key, shifts = "shift_stats", shifts + 1
                phase = "idle" if shifts % (a.steps + 1) == 0 else "adjoint"
            elif "chain_gather_kernel" in name:
                key, phase = "adjoint", "adjoint"
            elif "chain_partial_kernel" in name or "chain_apply_kernel" in name:
                key, phase = "direction_step", "primal"
            else:
                if phase == "idle" and "nchw_to_nhwc" in name:
                    phase = "primal"
                key = phase
            us[key] = us.get(key, 0.0) + dt
            cnt[key] = cnt.get(key, 0) + 1
        assert shifts == a.calls * (a.steps + 1), (shifts, a.calls, a.steps)
        # the primal phase holds steps + 1 passes per call (the last one forward only, for the final shift): reported per pass
        row.update(primal_us_per_pass=round(us.get("primal", 0) / (a.calls * (a.steps + 1)), 1), adjoint_us_per_step=round(us.get("adjoint", 0) / per, 1),
                   direction_step_us_per_step=round(us.get("direction_step", 0) / per, 2), shift_stats_us_per_state=round(us["shift_stats"] / shifts, 2),
                   launches={k: v for k, v in cnt.items() if k != "idle"}, outside_the_calls_us=round(us.get("idle", 0), 1))
        tot = sum(v for k, v in us.items() if k != "idle")
        row["new_kernels_share"] = round((us.get("direction_step", 0) + us["shift_stats"]) / tot, 5)
    else:
        row["device_us_per_chain_step"] = round(sum((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in ks) / (per * a.n[0]), 1)
    ht = _find(a.trace_dir, "hip_api_trace.csv")
    if ht:
        with open(ht) as fh:
            fn = [r["Function"] for r in csv.DictReader(fh)]
        row["host_syncs_per_call"] = {k: round(fn.count(k) / a.calls, 2) for k in ("hipStreamSynchronize", "hipDeviceSynchronize") if fn.count(k)}
    rows.append(row)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default="chain,job")
    ap.add_argument("--n", type=lambda s: [int(v) for v in s.split(",")], default=[1, 4, 8])
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--what", default="chain", choices=["chain", "composed"])
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--trace-dir", default="")
    ap.add_argument("--tmp", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = []
    for leg in a.leg.split(","):
        if leg == "chain":
            leg_chain(a, rows)
        elif leg == "job":
            import tempfile
            leg_job(a, rows, a.tmp or tempfile.mkdtemp())
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
