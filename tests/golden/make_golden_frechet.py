"""Generate the global-Frechet-basis fixture by RUNNING THE REFERENCE'S OWN DRIVER (build container only):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_frechet.py

``EditUncondDiffusion.run_edit_global_frechet_mean_zt`` (src/modules/edit.py:951-1246) in the manner of make_golden_transport.py, on the toy
``PullBackDDPM``, weights, scheduler and SPEC of transport_uncond_small.pt; the instance gets the attributes the method reads and __init__ never
defines (frechet_mean_space, h_t / h_t_idx, scheduler_name, edit_xt / edit_ht, use_x_space_guidance and the three regularisation switches).

The reference calls a compute_frechet_basis it never defines, so the global basis is pre-placed and the reference takes its load branch: four rank-4
local bases from the reference's own ``local_encoder_pullback_xt`` (min_iter=10, max_iter=50, thr=1e-4) at x_t(h_t) of four seeded Gaussian latents,
their Frechet mean by tests/_frechet_ref.py (float64, tol 1e-10), saved as [N, k] columns under the reference's names.  The sample's own basis is
pre-placed the same way.  Spaces x (vis_pc_list=[1]) and h (vis_num_pc=1), local_projection=True, pca_rank=4, eta = 1 tail off.

The reference's x-space run cannot reach its U-Net as written: with local_projection its projection_coeff plot evaluates ``u.T @ uk`` (edit.py:1168), and
uk is assigned in the h branch only -- an UnboundLocalError.  For the x run the method is compiled from its own source with that one plotting statement
removed (asserted to match exactly once); nothing else differs.  plt is replaced by a recorder of the savefig names.

Fixture (every file below 1 MiB)
  frechet_uncond_small.pt            cfg / seed / spectrum / args, x0 of the sample, the four latents, the local bases (u, s, vT) and the sample's own,
                                     the global bases u [N_h, 4] and v [N_x, 4] with the restatement's info, and per space: the (t, batch) of every
                                     U-Net call, the EXP_NAMEs, the projection_coeff names, the vk of every chain (from its first guidance call)
  frechet_uncond_small.saved.pt      per space, every tvu.save_image call (name, tensor) in order
  frechet_uncond_small.trace<i>.pt   the inputs of the U-Net calls of both runs (x then h), concatenated along the batch, 80 rows of 3 x 32 x 32 per file
"""
import contextlib
import inspect
import io
import os
import sys
import tempfile
import textwrap

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from make_golden import import_reference  # noqa: E402
from make_golden_edit import SPEC  # noqa: E402
import _frechet_ref as R  # noqa: E402

ROWS_PER_FILE = 80
PLOT_LINE = "plt.scatter(range(pca_rank), sorted((u.T @ uk).abs().tolist()), label='u')"


def main():
    torch.set_num_threads(8)
    ru, rd = import_reference()
    import modules.edit as redit
    from diffusion_pullback_amd import configs as cf
    from oracle import unet_ddpm

    saved, plots = [], []
    redit.tvu.save_image = lambda x, path, **kw: saved.append((os.path.basename(path), x.detach().clone()))
    redit.tqdm = lambda it, **kw: it

    class Plt:
        scatter = legend = close = staticmethod(lambda *a, **k: None)
        savefig = staticmethod(lambda path, **k: plots.append(os.path.basename(path)))
    redit.plt = Plt
    src = textwrap.dedent(inspect.getsource(redit.EditUncondDiffusion.run_edit_global_frechet_mean_zt))
    assert src.count(PLOT_LINE) == 1
    ns_x = {}
    exec(compile(src.replace(PLOT_LINE, "pass"), "<run_edit_global_frechet_mean_zt without the u plot>", "exec"), redit.__dict__, ns_x)
    run_x = ns_x["run_edit_global_frechet_mean_zt"]

    cwd = os.getcwd()
    os.chdir(tempfile.mkdtemp())                               # the driver writes ./inputs/... relative to the cwd
    os.makedirs("res", exist_ok=True); os.makedirs("obs", exist_ok=True)
    try:
        cfgd = dict(ch=32, ch_mult=(1, 2, 2), num_res_blocks=1, attn_resolutions=(16,), in_channels=3, out_ch=3, resolution=32)
        cfg = unet_ddpm.DDPMConfig(**cfgd)
        ns = ru.dict2namespace({"config": {"model": dict(ch=32, out_ch=3, ch_mult=[1, 2, 2], num_res_blocks=1, attn_resolutions=[16],
                                                       dropout=0.0, in_channels=3, resamp_with_conv=True), "data": dict(image_size=32)}})
        ns.device = "cpu"; ns.dtype = torch.float32
        net = rd.PullBackDDPM(ns).eval()
        net.load_state_dict(cf.ddpm_init_params(cfg, seed=3, spectrum=cf.Spectrum(**SPEC)), strict=True)
        trace = []
        fwd0 = net.forward

        def traced(x, t, *a, **k):
            trace.append((float(t), x.detach().clone()))
            return fwd0(x, t, *a, **k)

        class A:
            noise_schedule = None; device = "cpu"; dtype = torch.float32
        args = dict(for_steps=20, inv_steps=20, h_t=0.8, edit_t=0.6, x_space_guidance_edit_step=1.0, x_space_guidance_scale=0.1,
                    x_space_guidance_num_step=8, vis_num=4, pca_rank=4, num_local_basis=4, idx=0, seed=0, rng_seed=53, scheduler_name="yh_custom",
                    dataset_name="CelebA_HQ", model_name="CelebA_HQ_HF", runs=dict(x=dict(vis_num_pc=None, vis_pc_list=[1]), h=dict(vis_num_pc=1, vis_pc_list=None)))
        x0 = {0: torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(31)).clamp(-1, 1)}
        latents = [torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(700 + i)) for i in range(args["num_local_basis"])]
        eu = object.__new__(redit.EditUncondDiffusion)
        eu.pca_device = eu.buffer_device = "cpu"; eu.memory_bound = 50; eu.device = "cpu"; eu.dtype = torch.float32; eu.seed = 0
        eu.save_result_as = "image"; eu.unet = net; eu.scheduler = ru.YHCustomScheduler(A()); eu.model_name = args["model_name"]
        eu.image_size = 32; eu.c_in = 3; eu.dataset = x0; eu.dataset_name = args["dataset_name"]
        eu.for_steps, eu.inv_steps, eu.use_yh_custom_scheduler, eu.edit_t, eu.h_t = 20, 20, True, 0.6, 0.8
        eu.scheduler.set_timesteps(eu.for_steps, device="cpu")
        eu.edit_t_idx = (eu.scheduler.timesteps - eu.edit_t * 1000).abs().argmin()
        eu.h_t_idx = (eu.scheduler.timesteps - eu.h_t * 1000).abs().argmin()
        eu.performance_boosting_t_idx = 1000                   # eta = 1 tail off: its noise is a device RNG draw, not reproducible
        eu.use_x_space_guidance = True; eu.edit_xt = "parallel-x"; eu.edit_ht = "default"; eu.scheduler_name = args["scheduler_name"]
        eu.use_dynamic_thresholding = eu.use_preserve_contrast = eu.use_preserve_norm = False
        eu.x_space_guidance_edit_step, eu.x_space_guidance_scale, eu.x_space_guidance_num_step = 1.0, 0.1, 8
        eu.result_folder, eu.obs_folder = "res", "obs"

        # the four local bases and the sample's own, by the reference's pullback at x_t(h_t)
        torch.manual_seed(args["rng_seed"])
        pull = lambda xt, t: net.local_encoder_pullback_xt(x=xt, t=t, op="mid", block_idx=0, pca_rank=args["pca_rank"], min_iter=10, max_iter=50,
                                                           convergence_threshold=1e-4)
        with contextlib.redirect_stdout(io.StringIO()):
            local = []
            for xT in latents:
                xt, t, _ = eu.DDIMforwardsteps(xT, t_start_idx=0, t_end_idx=eu.h_t_idx)
                local.append(tuple(z.clone() for z in pull(xt, t)))
            xT = eu.run_DDIMinversion(idx=0)
            xt, t, _ = eu.DDIMforwardsteps(xT, t_start_idx=0, t_end_idx=eu.h_t_idx)
            own = tuple(z.clone() for z in pull(xt, t))
        d_own = "./inputs/local_encoder_pullback_uncond-model_CelebA_HQ_HF-dataset_CelebA_HQ-scheduler_yh_custom-num_steps_20-pca_rank_4"
        d_glob = "./inputs/global_frechet_mean_uncond-model_CelebA_HQ_HF-dataset_CelebA_HQ-scheduler_yh_custom-num_steps_20-pca_rank_4"
        os.makedirs(d_own, exist_ok=True); os.makedirs(d_glob, exist_ok=True)
        torch.save(own[0], os.path.join(d_own, "u-xt-CelebA_HQ_0-0.8T-mid-block_0-seed_0.pt"))
        torch.save(own[2], os.path.join(d_own, "vT-xt-CelebA_HQ_0-0.8T-mid-block_0-seed_0.pt"))

        # the global bases: the restatement's mean of the four, [N, k] columns under the reference's names
        glob, ginfo = {}, {}
        for space, stack in (("x", np.stack([b[2].numpy() for b in local])), ("h", np.stack([b[0].numpy().T for b in local]))):
            y, info = R.frechet_mean_ref(stack, tol=1e-10, max_iter=2000)
            assert info["converged"], space
            glob[space] = torch.from_numpy(y.T.copy()).float()
            ginfo[space] = dict(iterations=info["iterations"], grad_norm=info["grad_norm"], cost=info["cost"], weight=info["weight"], theta=info["theta"])
            torch.save(glob[space], os.path.join(d_glob, ("v-" if space == "x" else "u-") + "0.8T-mid-block_0-seed_0-num_local_basis_4.pt"))

        net.forward = traced
        runs = {}
        for space in ("x", "h"):
            saved.clear(); plots.clear(); n0 = len(trace)
            eu.frechet_mean_space = space
            call = (lambda **k: run_x(eu, **k)) if space == "x" else eu.run_edit_global_frechet_mean_zt
            kw = dict(idx=0, op="mid", block_idx=0, vis_num=4, pca_rank=4, num_local_basis=4, local_projection=True, **args["runs"][space])
            with contextlib.redirect_stdout(io.StringIO()):
                call(**kw)
            calls = trace[n0:]
            step = args["x_space_guidance_edit_step"]
            first = [x for t, x in calls if x.shape[0] == 2][::args["x_space_guidance_num_step"]]        # each chain's first guidance call
            names = [n[len("x0_gen-"):-len(".png")] for n, _ in saved if n.startswith("x0_gen-xt-")]
            assert len(first) == len(names) == 2, (len(first), names)
            runs[space] = dict(trace_t=[t for t, _ in calls], trace_batch=[int(x.shape[0]) for _, x in calls], saved=[(n, x) for n, x in saved],
                               plots=list(plots), names=names, vk=[((x[1] - x[0]) / step).reshape(-1).clone() for x in first])
            n_saved, n_calls = len(saved), len(trace)
            with contextlib.redirect_stdout(io.StringIO()):   # a second call runs no experiment once the pictures exist (save_image is captured: touch them)
                for n, _ in saved:
                    if n.startswith("x0_gen-"):
                        open(os.path.join("res", n), "w").close()
                call(**kw)
            runs[space]["second_call_unet_calls"] = len(trace) - n_calls       # the reference's job-level check looks for a name without x0_gen-: it re-runs the inversion
            assert len(saved) - n_saved == sum(1 for n, _ in saved[n_saved:] if not n.startswith("x0_gen-xt-")), "an experiment ran twice"
            del trace[n_calls:]
            for n, _ in saved:                                 # the h run starts clean
                if n.startswith("x0_gen-") and os.path.exists(os.path.join("res", n)):
                    os.remove(os.path.join("res", n))

        rows = torch.cat([x for _, x in trace], dim=0)
        fix = dict(cfg=cfgd, seed=3, spectrum=SPEC, args=args, x0=x0[0], latents=latents, local_u=[b[0] for b in local], local_s=[b[1] for b in local],
                   local_vT=[b[2] for b in local], own_u=own[0], own_s=own[1], own_vT=own[2], global_u=glob["h"], global_v=glob["x"], global_info=ginfo,
                   h_t_idx=int(eu.h_t_idx), edit_t_idx=int(eu.edit_t_idx), runs=runs, trace_files=[], dirs=dict(own=d_own, glob=d_glob))
        for old in os.listdir(HERE):
            if old.startswith("frechet_uncond_small.trace"):
                os.remove(os.path.join(HERE, old))
        for i, r0 in enumerate(range(0, rows.shape[0], ROWS_PER_FILE)):
            fn = f"frechet_uncond_small.trace{i}.pt"
            torch.save(rows[r0:r0 + ROWS_PER_FILE].clone(), os.path.join(HERE, fn))
            fix["trace_files"].append(fn)
        torch.save({space: runs[space].pop("saved") for space in ("x", "h")}, os.path.join(HERE, "frechet_uncond_small.saved.pt"))
        torch.save(fix, os.path.join(HERE, "frechet_uncond_small.pt"))
        for space in ("x", "h"):
            r = runs[space]
            print(space, "unet calls", len(r["trace_t"]), "rows", sum(r["trace_batch"]), "names", r["names"], "plots", r["plots"],
                  "second call", r["second_call_unet_calls"], "mean steps", ginfo[space]["iterations"], "theta max", float(np.max(ginfo[space]["theta"])))
    finally:
        os.chdir(cwd)
    for f in sorted(os.listdir(HERE)):
        if f.startswith("frechet_uncond_small"):
            print(f, os.path.getsize(os.path.join(HERE, f)))


if __name__ == "__main__":
    main()
