"""Generate the global-Hungarian-basis fixture by RUNNING THE REFERENCE'S OWN DRIVER (build container only):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_hungarian.py

``EditUncondDiffusion.run_edit_global_hungarian_mean_zt`` (src/modules/edit.py:1249-1514) in the manner of make_golden_frechet.py, on the toy
``PullBackDDPM``, weights, scheduler, sample, latents and local bases of frechet_uncond_small.pt (read from that fixture, not stored again); the
instance gets the attributes the method reads and __init__ never defines (h_t / h_t_idx, scheduler_name, edit_xt / edit_ht, use_x_space_guidance
and the three regularisation switches).

The reference calls a compute_hungarian_basis it never defines, so both global bases are pre-placed and the reference takes its load branch: the
Hungarian-matched means of the four local bases by tests/_hungarian_ref.py (float64, '1/cosine', anchor 0), u from the stack of u^T and v from the
stack of vT, saved as [N, k] columns under the reference's names.  The sample's own basis is pre-placed the same way.  The method has one live path
(x-space guidance along v, edit.py:1422-1468); it runs once, vis_pc_list=[1], local_projection=True, pca_rank=4, eta = 1 tail off.  plt is replaced
by a recorder of the savefig names.

Fixture (every file below 1 MiB)
  hungarian_uncond_small.pt            args, the global bases u [N_h, 4] and v [N_x, 4] with the restatement's perm / sign / cost / weight, the
                                       (t, batch) of every U-Net call, the EXP_NAMEs, the projection_coeff names, the vk of every chain
  hungarian_uncond_small.saved.pt      every tvu.save_image call (name, tensor) in order
  hungarian_uncond_small.trace<i>.pt   the inputs of the U-Net calls, concatenated along the batch, 80 rows of 3 x 32 x 32 per file
"""
import contextlib
import io
import os
import sys
import tempfile

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from make_golden import import_reference  # noqa: E402
import _hungarian_ref as R  # noqa: E402

ROWS_PER_FILE = 80


def main():
    torch.set_num_threads(8)
    ru, rd = import_reference()
    import modules.edit as redit
    from diffusion_pullback_amd import configs as cf
    from oracle import unet_ddpm

    f = torch.load(os.path.join(HERE, "frechet_uncond_small.pt"), weights_only=False)
    fa = f["args"]
    saved, plots = [], []
    redit.tvu.save_image = lambda x, path, **kw: saved.append((os.path.basename(path), x.detach().clone()))
    redit.tqdm = lambda it, **kw: it

    class Plt:
        scatter = legend = close = staticmethod(lambda *a, **k: None)
        savefig = staticmethod(lambda path, **k: plots.append(os.path.basename(path)))
    redit.plt = Plt

    cwd = os.getcwd()
    os.chdir(tempfile.mkdtemp())                               # the driver writes ./inputs/... relative to the cwd
    os.makedirs("res", exist_ok=True); os.makedirs("obs", exist_ok=True)
    try:
        cfg = unet_ddpm.DDPMConfig(**f["cfg"])
        ns = ru.dict2namespace({"config": {"model": dict(ch=32, out_ch=3, ch_mult=[1, 2, 2], num_res_blocks=1, attn_resolutions=[16],
                                                       dropout=0.0, in_channels=3, resamp_with_conv=True), "data": dict(image_size=32)}})
        ns.device = "cpu"; ns.dtype = torch.float32
        net = rd.PullBackDDPM(ns).eval()
        net.load_state_dict(cf.ddpm_init_params(cfg, seed=f["seed"], spectrum=cf.Spectrum(**f["spectrum"])), strict=True)
        trace = []
        fwd0 = net.forward

        def traced(x, t, *a, **k):
            trace.append((float(t), x.detach().clone()))
            return fwd0(x, t, *a, **k)

        class A:
            noise_schedule = None; device = "cpu"; dtype = torch.float32
        args = {k: fa[k] for k in ("for_steps", "inv_steps", "h_t", "edit_t", "x_space_guidance_edit_step", "x_space_guidance_scale",
                                   "x_space_guidance_num_step", "vis_num", "pca_rank", "num_local_basis", "idx", "seed", "scheduler_name",
                                   "dataset_name", "model_name")}
        args.update(rng_seed=59, distance="1/cosine", run=dict(vis_num_pc=None, vis_pc_list=[1]))
        eu = object.__new__(redit.EditUncondDiffusion)
        eu.pca_device = eu.buffer_device = "cpu"; eu.memory_bound = 50; eu.device = "cpu"; eu.dtype = torch.float32; eu.seed = 0
        eu.save_result_as = "image"; eu.unet = net; eu.scheduler = ru.YHCustomScheduler(A()); eu.model_name = args["model_name"]
        eu.image_size = 32; eu.c_in = 3; eu.dataset = {0: f["x0"]}; eu.dataset_name = args["dataset_name"]
        eu.for_steps, eu.inv_steps, eu.use_yh_custom_scheduler, eu.edit_t, eu.h_t = 20, 20, True, args["edit_t"], args["h_t"]
        eu.scheduler.set_timesteps(eu.for_steps, device="cpu")
        eu.edit_t_idx = (eu.scheduler.timesteps - eu.edit_t * 1000).abs().argmin()
        eu.h_t_idx = (eu.scheduler.timesteps - eu.h_t * 1000).abs().argmin()
        eu.performance_boosting_t_idx = 1000                   # eta = 1 tail off: its noise is a device RNG draw, not reproducible
        eu.use_x_space_guidance = True; eu.edit_xt = "parallel-x"; eu.edit_ht = "default"; eu.scheduler_name = args["scheduler_name"]
        eu.use_dynamic_thresholding = eu.use_preserve_contrast = eu.use_preserve_norm = False
        eu.x_space_guidance_edit_step, eu.x_space_guidance_scale, eu.x_space_guidance_num_step = 1.0, 0.1, 8
        eu.result_folder, eu.obs_folder = "res", "obs"

        d_own = "./inputs/local_encoder_pullback_uncond-model_CelebA_HQ_HF-dataset_CelebA_HQ-scheduler_yh_custom-num_steps_20-pca_rank_4"
        d_glob = "./inputs/global_hungarian_mean_uncond-model_CelebA_HQ_HF-dataset_CelebA_HQ-scheduler_yh_custom-num_steps_20-pca_rank_4"
        os.makedirs(d_own, exist_ok=True); os.makedirs(d_glob, exist_ok=True)
        torch.save(f["own_u"], os.path.join(d_own, "u-xt-CelebA_HQ_0-0.8T-mid-block_0-seed_0.pt"))
        torch.save(f["own_vT"], os.path.join(d_own, "vT-xt-CelebA_HQ_0-0.8T-mid-block_0-seed_0.pt"))

        # the global bases: the restatement's matched means of the four, [N, k] columns under the reference's names
        glob, ginfo = {}, {}
        for tag, stack in (("u", np.stack([u.numpy().T for u in f["local_u"]])), ("v", np.stack([v.numpy() for v in f["local_vT"]]))):
            y, info = R.hungarian_mean_ref(stack, init=0, distance=args["distance"])
            assert info["converged"], tag
            glob[tag] = torch.from_numpy(y.T.copy()).float()
            ginfo[tag] = {k: info[k] for k in ("perm", "sign", "cost", "sweeps", "changed", "weight")}
            torch.save(glob[tag], os.path.join(d_glob, f"{tag}-0.8T-mid-block_0-seed_0.pt"))

        net.forward = traced
        torch.manual_seed(args["rng_seed"])
        kw = dict(idx=0, op="mid", block_idx=0, vis_num=4, pca_rank=4, num_local_basis=4, local_projection=True, **args["run"])
        with contextlib.redirect_stdout(io.StringIO()):
            eu.run_edit_global_hungarian_mean_zt(**kw)
        step = args["x_space_guidance_edit_step"]
        first = [x for t, x in trace if x.shape[0] == 2][::args["x_space_guidance_num_step"]]        # each chain's first guidance call
        names = [n[len("x0_gen-"):-len(".png")] for n, _ in saved if n.startswith("x0_gen-xt-")]
        assert len(first) == len(names) == 2, (len(first), names)
        run = dict(trace_t=[t for t, _ in trace], trace_batch=[int(x.shape[0]) for _, x in trace], plots=list(plots), names=names,
                   vk=[((x[1] - x[0]) / step).reshape(-1).clone() for x in first])
        rows = torch.cat([x for _, x in trace], dim=0)
        fix = dict(args=args, global_u=glob["u"], global_v=glob["v"], global_info=ginfo, run=run, trace_files=[], dirs=dict(own=d_own, glob=d_glob),
                   base="frechet_uncond_small.pt")
        for old in os.listdir(HERE):
            if old.startswith("hungarian_uncond_small.trace"):
                os.remove(os.path.join(HERE, old))
        for i, r0 in enumerate(range(0, rows.shape[0], ROWS_PER_FILE)):
            fn = f"hungarian_uncond_small.trace{i}.pt"
            torch.save(rows[r0:r0 + ROWS_PER_FILE].clone(), os.path.join(HERE, fn))
            fix["trace_files"].append(fn)
        torch.save([(n, x) for n, x in saved], os.path.join(HERE, "hungarian_uncond_small.saved.pt"))
        torch.save(fix, os.path.join(HERE, "hungarian_uncond_small.pt"))
        print("unet calls", len(run["trace_t"]), "rows", sum(run["trace_batch"]), "names", run["names"], "plots", run["plots"],
              "sweeps", {t: ginfo[t]["sweeps"] for t in ginfo}, "perm v", ginfo["v"]["perm"].tolist(), "sign v", ginfo["v"]["sign"].tolist())
    finally:
        os.chdir(cwd)
    for fn in sorted(os.listdir(HERE)):
        if fn.startswith("hungarian_uncond_small"):
            print(fn, os.path.getsize(os.path.join(HERE, fn)))


if __name__ == "__main__":
    main()
