"""Not a test: times principal geodesic analysis (dpb_pga_tangent_gram / _eig / _combine) on the Frechet benchmark's set, B = 100 local bases of k = 50 rows.
    python tools/gpu_pga_bench.py [--n 16384,32768,81920,196608] [--b 100] [--k 50] [--modes 16] [--reps 5] [--out FILE.jsonl]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/gpu_pga_bench.py --leg trace --n-one 16384
    python tools/gpu_pga_bench.py --leg split --stats DIR/.../t_kernel_stats.csv --n-one 16384 [--out FILE.jsonl]
The set: per basis 10 directions shared by all and 40 of its own, Gaussian rows (tools/gpu_frechet_bench.py).  The base is the flag mean: central, so every member is inside the
log map's domain (by 6e-6 rad on this set of 40 own random directions per member -- `largest_angle`), which a member as the base is not.  Every size runs in a fresh child process under its own time limit; the first
that fails or runs out of time ends the run.  One JSON line per size; every time is the median of --reps after a warm-up, device-synchronised:
  copy_gbytes_per_s     a device-to-device copy of 1 GiB, bytes read plus bytes written over its time
  base_ms               the base point: dpb_frechet_init (the cross-Gram pass over X), the flag solve on its Gram, dpb_frechet_start, dpb_frechet_finish
  tangent_gram_ms       dpb_pga_tangent_gram: M = C Ghat, the B log maps, the B (B + 1) / 2 pair workgroups -- one pass over Ghat
  eig_ms                dpb_pga_eig (the centring and the eigen-solve; route in `solver`)
  combine_ms            dpb_pga_combine of modes + the mean tangent: the coefficient matrices and ceil(J k / 64) passes over X; combine_x_gbytes_per_s
                        counts the bytes of X once per pass plus the output
  call_ms               geometry.grassmann_pga end to end (its host reads included)
  torch_fp64_ms         the float64 torch composition of tests/_pga_ref.py on the same GPU at the same base: batched qr, svd log maps, the flattened
                        B x kN matrix, eigh of its centred B x B Gram, one matmul for the modes
  gram_rel_err, variance_rel_err, modes_rel_err, scores_rel_err   this library against that composition (max |diff| over max |ref|; modes: Frobenius)
The split of a call into the pair kernel, the eigen-solve and the stream comes from a rocprofv3 run of its own (legs `trace` and `split`), with a device
copy of X's bytes in the same trace for scale."""
import argparse
import csv
import ctypes as C
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
    return statistics.median(ts), [round(x * 1e3, 3) for x in ts]


def _set(b, k, n, shared=10, seed=97):
    import torch
    g = torch.Generator(device=DEV).manual_seed(seed)
    common = torch.randn(shared, n, generator=g, device=DEV)
    x = torch.randn(b, k, n, generator=g, device=DEV)
    x[:, :shared] = common
    return x


class _Pga:
    """the entry points on their two scratch blocks, phase by phase (what geometry.grassmann_pga(base="flag") calls)"""

    def __init__(self, x, modes):
        import torch
        from diffusion_pullback_amd import lib as L
        self.L, self.lib, self.x, self.m = L, L.load(), x, modes
        self.b, self.k, self.n = x.shape
        b, k, n, lib = self.b, self.k, self.n, self.lib
        self.rows = modes + 1
        self.fneed = int(lib.dpb_frechet_scratch_bytes(b, k, n, 0))
        self.sneed = int(lib.dpb_flag_mean_solver_bytes(b, k, k, 64))
        self.pneed = int(lib.dpb_pga_scratch_bytes(b, b, k, n, self.rows))
        assert self.fneed and self.sneed and self.pneed
        u8 = lambda nbytes: torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        self.fs, self.ss, self.ps = u8(self.fneed), u8(self.sneed), u8(self.pneed)
        self.st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=DEV)
        f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=DEV)
        self.Y, self.weight, self.theta = f32(k, n), f32(k), f32(b, k)
        self.info, self.fCt, self.finfo = f64(8 + 1 + b), f64(b * k, k), f64(72 + b)
        self.T, self.state, self.Wt = f64(b, b), torch.empty(b, dtype=torch.int32, device=DEV), torch.zeros(self.rows, b, dtype=torch.float64, device=DEV)
        self.out, self.tangents = f64(72 + b * modes + b), f32(self.rows, k, n)

    def base(self):
        lib, b, k, n, ck = self.lib, self.b, self.k, self.n, self.L.check
        ck(lib.dpb_frechet_init(self.x.data_ptr(), b, k, n, 0, 0, self.fs.data_ptr(), self.fneed, self.st))
        ghat = lib.dpb_frechet_ghat(b, k, n, 0, self.fs.data_ptr())
        ck(lib.dpb_flag_mean_init(None, ghat, b, k, n, k, 0, 64, self.ss.data_ptr(), self.sneed, self.st))
        ck(lib.dpb_flag_mean_iterate(64, 1e-10, ghat, b, k, n, k, 64, self.ss.data_ptr(), self.sneed, self.st))
        ck(lib.dpb_flag_mean_finish(None, ghat, None, self.weight.data_ptr(), self.theta.data_ptr(), self.fCt.data_ptr(), self.finfo.data_ptr(), b, k, n, k, 64,
                                    self.ss.data_ptr(), self.sneed, self.st))
        ck(lib.dpb_frechet_start(self.fCt.data_ptr(), b, k, n, 0, self.fs.data_ptr(), self.fneed, self.st))
        ck(lib.dpb_frechet_finish(self.x.data_ptr(), self.Y.data_ptr(), self.weight.data_ptr(), self.theta.data_ptr(), self.info.data_ptr(), b, k, n, 0,
                                  self.fs.data_ptr(), self.fneed, self.st))

    def gram(self):
        self.L.check(self.lib.dpb_pga_tangent_gram(self.b, self.b, self.k, self.n, 0, self.rows, self.fs.data_ptr(), self.fneed, self.T.data_ptr(),
                                                   self.theta.data_ptr(), self.state.data_ptr(), self.ps.data_ptr(), self.pneed, self.st))

    def eig(self):
        self.L.check(self.lib.dpb_pga_eig(self.T.data_ptr(), self.b, self.b, self.k, self.n, self.rows, self.m, 1, self.Wt.data_ptr(), self.out.data_ptr(),
                                          self.ps.data_ptr(), self.pneed, self.st))

    def combine(self):
        self.Wt[self.m] = 1.0 / self.b
        self.L.check(self.lib.dpb_pga_combine(self.x.data_ptr(), self.Wt.data_ptr(), self.rows, self.tangents.data_ptr(), self.b, self.b, self.k, self.n, 0,
                                              self.rows, self.fs.data_ptr(), self.fneed, self.ps.data_ptr(), self.pneed, self.st))


def _torch_pga(x, y, modes):
    """tests/_pga_ref.py in float64 torch at the base y [k, N] (orthonormal rows): (T, variance, modes [M, kN], scores)"""
    import torch as t
    q = t.linalg.qr(x.double().transpose(1, 2)).Q.transpose(1, 2)
    u, c, wt = t.linalg.svd(y @ q.transpose(1, 2))
    d = wt @ q - c[:, :, None] * (u.transpose(1, 2) @ y)
    s = d.norm(dim=2)
    scale = t.where(s > 0, t.atan2(s, c) / s.clamp_min(1e-300), t.zeros_like(s))
    flat = (u @ (scale[:, :, None] * d)).reshape(x.shape[0], -1)
    gram = flat @ flat.T
    cen = flat - flat.mean(dim=0)
    lam, vec = t.linalg.eigh(cen @ cen.T)
    lam, vec = lam.flip(0)[:modes], vec.flip(1)[:, :modes]
    md = (vec / lam.sqrt()).T @ cen
    return gram, lam / x.shape[0], md, cen @ md.T


def _size_leg(a):
    import torch
    from diffusion_pullback_amd import geometry
    b, k, n, m = a.b, a.k, a.n_one, a.modes
    rec = dict(leg="size", B=b, k=k, N=n, modes=m, seed=a.seed, R=b * k, x_gbytes=round(4.0 * b * k * n / 1e9, 3), ghat_gbytes=round(8.0 * (b * k) ** 2 / 1e9, 3))
    src = torch.empty(1 << 28, dtype=torch.float32, device=DEV)
    dst = torch.empty_like(src)
    dt, _ = _timed(lambda: dst.copy_(src), a.reps)
    rec["copy_gbytes_per_s"] = round(2.0 * src.numel() * 4 / dt / 1e9, 1)
    del src, dst
    x = _set(b, k, n, seed=a.seed)
    p = _Pga(x, m)
    for name, fn in (("base", p.base), ("tangent_gram", p.gram), ("eig", p.eig), ("combine", p.combine)):
        dt, runs = _timed(fn, a.reps)
        rec.update({name + "_ms": round(dt * 1e3, 3), name + "_ms_runs": runs})
    passes = (p.rows * k + 63) // 64
    rec.update(combine_passes=passes, combine_x_gbytes_per_s=round((passes * 4.0 * b * k * n + 4.0 * p.rows * k * n) / (rec["combine_ms"] * 1e-3) / 1e9, 1))
    head = p.out[:72].cpu().numpy()
    rec.update(solver={1: "jacobi", 2: "subspace"}[int(head[3])], valid_members=int(head[0]), largest_angle=float(p.theta.max()),
               total_variance=float(head[1]), explained=float(head[8:8 + m].sum() / head[1]))
    dt, runs = _timed(lambda: geometry.grassmann_pga(x, base="flag", n_modes=m), a.reps)
    rec.update(call_ms=round(dt * 1e3, 3), call_ms_runs=runs)
    yd = p.Y.double()
    lam, v = torch.linalg.eigh(yd @ yd.T)
    y = (v / lam.sqrt()) @ v.T @ yd                                      # the polar factor: the returned rows made orthonormal in float64
    dt, runs = _timed(lambda: _torch_pga(x, y, m), min(a.reps, 3))
    rec.update(torch_fp64_ms=round(dt * 1e3, 1), torch_fp64_ms_runs=runs)
    gram, var, md, sc = _torch_pga(x, y, m)
    ours = p.tangents[:m].double().reshape(m, -1)
    sign = torch.sign((ours * md).sum(dim=1))
    scores = p.out[72:72 + b * m].view(b, m)
    rec.update(gram_rel_err=float((p.T - gram).abs().max() / gram.abs().max()), variance_rel_err=float((torch.from_numpy(head[8:8 + m]).to(DEV) - var).abs().max() / var.max()),
               modes_rel_err=float((ours - sign[:, None] * md).norm(dim=1).max()), scores_rel_err=float((scores - sc * sign).abs().max() / sc.abs().max()))
    print(json.dumps(rec), flush=True)


def _trace_leg(a):
    """the work a kernel trace is taken of: the base, the three phases once, and a device copy of X's bytes for scale"""
    import torch
    x = _set(a.b, a.k, a.n_one, seed=a.seed)
    p = _Pga(x, a.modes)
    p.base(); p.gram(); p.eig(); p.combine()
    torch.empty_like(x).copy_(x)
    torch.cuda.synchronize()


def _split_leg(a):
    rows = list(csv.DictReader(open(a.stats)))
    fam, calls = {}, {}
    for r in rows:
        name, ns, c = r["Name"], float(r["TotalDurationNs"]), int(r["Calls"])
        key = ("pair" if "pga_pair_kernel" in name else "member_log_maps" if "pga_member_kernel" in name else "m_product" if "pga_product_kernel" in name else
               "eig_jacobi" if "pga_jacobi_kernel" in name else "eig_rest" if any(s in name for s in ("pga_rowsum", "pga_head", "pga_center", "pga_post", "pga_pack")) else
               "base_flag_solve" if "fm_" in name else "base_cross_gram" if "cross_gram_kernel" in name else
               "coefficients" if ("pga_coef_kernel" in name or "pga_ksum_kernel" in name) else "stream" if "fr_stream_kernel" in name else
               "device_copy" if "copyBuffer" in name else "other")
        if key == "device_copy":                               # the copy of X is the longest one (dpb_pga_tangent_gram copies the members' state too)
            ns = float(r["MaxNs"])
            fam[key] = 0.0
        fam[key] = fam.get(key, 0.0) + ns
        calls[key] = calls.get(key, 0) + c
    R_ = a.b * a.k
    ms = lambda key: round(fam.get(key, 0.0) / 1e6, 4)
    rec = dict(leg="split", B=a.b, k=a.k, N=a.n_one, modes=a.modes, source="rocprofv3 --kernel-trace --stats", pair_ms=ms("pair"),
               pair_ghat_gbytes_per_s=round(8.0 * R_ * R_ / 2 / max(fam.get("pair", 0.0), 1.0), 1), member_log_maps_ms=ms("member_log_maps"), m_product_ms=ms("m_product"),
               eig_jacobi_ms=ms("eig_jacobi"), eig_rest_ms=ms("eig_rest"), base_flag_solve_ms=ms("base_flag_solve"), base_cross_gram_ms=ms("base_cross_gram"),
               coefficients_ms=ms("coefficients"), stream_ms=ms("stream"),
               stream_launches=calls.get("stream", 0), stream_x_gbytes_per_s=round(calls.get("stream", 0) * 4.0 * R_ * a.n_one / max(fam.get("stream", 0.0), 1.0), 1),
               device_copy_ms=ms("device_copy"), device_copy_gbytes_per_s=round(2 * 4.0 * R_ * a.n_one / max(fam.get("device_copy", 0.0), 1.0), 1))
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="16384,32768,81920,196608")
    ap.add_argument("--b", type=int, default=100)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--modes", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=97)
    ap.add_argument("--leg-timeout", type=int, default=240)
    ap.add_argument("--out", default="")
    ap.add_argument("--stats", default="")
    ap.add_argument("--leg", default="", help=argparse.SUPPRESS)
    ap.add_argument("--n-one", type=int, default=16384, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return {"size": _size_leg, "trace": _trace_leg, "split": _split_leg}[a.leg](a)
    for n in a.n.split(","):
        cmd = ["timeout", "-k", "10", str(a.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", "size", "--n-one", n, "--b", str(a.b),
               "--k", str(a.k), "--modes", str(a.modes), "--reps", str(a.reps), "--seed", str(a.seed)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:                     # a fault, an abort or a time limit: nothing more is started on the GPU
            print(json.dumps(dict(leg="size", N=int(n), failed=True, returncode=r.returncode, stderr=r.stderr[-800:])), flush=True)
            sys.exit(1)
        print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(lines[-1] + "\n")


if __name__ == "__main__":
    main()
