"""Generate the parallel-transport fixture by RUNNING THE REFERENCE'S OWN DRIVER (build container only):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_transport.py

``EditUncondDiffusion.run_edit_parallel_transport`` (src/modules/edit.py:782-948) in the manner of make_golden_edit.py: the instance is created with
``object.__new__`` and given the attributes __init__ would set (plus h_t / h_t_idx / edit_xt / edit_ht / scheduler_name, which the method reads and
__init__ leaves commented out or never defines), on the same toy ``PullBackDDPM``, weights, scheduler and SPEC as edit_uncond_small.pt.

The two bases come from the reference's ``local_encoder_pullback_xt`` at rank 4 (min_iter=10, max_iter=50, thr=1e-4, the job's own constants), at the
x_t(h_t) the job itself reaches, and are pre-placed under the names the job loads: the reference then runs its normalising load branch, and its
``assert pca_rank == 50`` is met by the call argument (the directory name carries 50, the files rank 4).  eta = 1 tail off, as in edit_uncond_small.

Fixture (every file below 1 MiB)
  transport_uncond_small.pt            cfg / seed / spectrum / args, x0 of both samples, the four basis tensors (+ s), h_t_idx / edit_t_idx, the (t, batch)
                                       of every U-Net call, every tvu.save_image call (name, tensor) in order -- the vk- tensors
                                       [+transported, -transported, +original, -original] included --, the basis file names
  transport_uncond_small.trace<i>.pt   the inputs of the 212 U-Net calls, concatenated along the batch in call order, 80 rows of 3 x 32 x 32 per file
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
sys.path.insert(0, os.path.join(HERE, "..", ".."))

import torch  # noqa: E402

from make_golden import import_reference  # noqa: E402
from make_golden_edit import SPEC  # noqa: E402

ROWS_PER_FILE = 80


def main():
    torch.set_num_threads(8)
    ru, rd = import_reference()
    import modules.edit as redit
    from diffusion_pullback_amd import configs as cf
    from oracle import unet_ddpm

    saved = []
    redit.tvu.save_image = lambda x, path, **kw: saved.append((os.path.basename(path), x.detach().clone()))
    redit.tqdm = lambda it, **kw: it
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
                    x_space_guidance_num_step=8, vis_num=4, vis_num_pc=2, pca_rank=4, sample_idx_0=0, sample_idx_1=1, seed=0, rng_seed=47,
                    scheduler_name="yh_custom", dataset_name="CelebA_HQ", model_name="CelebA_HQ_HF")
        x0 = {i: torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(31 + i)).clamp(-1, 1) for i in (0, 1)}
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
        eu.x_space_guidance_edit_step, eu.x_space_guidance_scale, eu.x_space_guidance_num_step = 1.0, 0.1, 8
        eu.result_folder, eu.obs_folder = "res", "obs"

        # the two bases, by the reference's own pullback at the job's x_t(h_t), pre-placed under the names the job loads
        d = ("./inputs/local_encoder_pullback_uncond-model_CelebA_HQ_HF-dataset_CelebA_HQ-scheduler_yh_custom-num_steps_20-pca_rank_50")
        os.makedirs(d, exist_ok=True)
        torch.manual_seed(args["rng_seed"])
        basis = {}
        with contextlib.redirect_stdout(io.StringIO()):
            for i in (0, 1):
                xT = eu.run_DDIMinversion(idx=i)
                xt, t, _ = eu.DDIMforwardsteps(xT, t_start_idx=0, t_end_idx=eu.h_t_idx)
                u, s, vT = net.local_encoder_pullback_xt(x=xt, t=t, op="mid", block_idx=0, pca_rank=args["pca_rank"], min_iter=10, max_iter=50,
                                                         convergence_threshold=1e-4)
                basis[i] = (u.clone(), s.clone(), vT.clone())
                name = f"xt-CelebA_HQ_{i}-0.8T-mid-block_0-seed_0.pt"
                torch.save(u, os.path.join(d, "u-" + name)); torch.save(vT, os.path.join(d, "vT-" + name))
        saved.clear()

        net.forward = traced
        with contextlib.redirect_stdout(io.StringIO()):
            eu.run_edit_parallel_transport(sample_idx_0=0, sample_idx_1=1, op="mid", block_idx=0, vis_num=4, vis_num_pc=2, pca_rank=50)
        n_saved = len(saved)
        n_calls = len(trace)
        with contextlib.redirect_stdout(io.StringIO()):       # a second call does nothing once the pictures exist (save_image is captured: touch them)
            for n, _ in saved:
                if n.startswith("x0_gen-"):
                    open(os.path.join("res", n), "w").close()
            eu.run_edit_parallel_transport(sample_idx_0=0, sample_idx_1=1, op="mid", block_idx=0, vis_num=4, vis_num_pc=2, pca_rank=50)
        assert len(saved) == n_saved and len(trace) == n_calls, "the reference's skip rule did not hold"

        rows = torch.cat([x for _, x in trace], dim=0)
        fix = dict(cfg=cfgd, seed=3, spectrum=SPEC, args=args, x0=[x0[0], x0[1]], u=[basis[0][0], basis[1][0]], s=[basis[0][1], basis[1][1]],
                   vT=[basis[0][2], basis[1][2]], h_t_idx=int(eu.h_t_idx), edit_t_idx=int(eu.edit_t_idx), trace_t=[t for t, _ in trace],
                   trace_batch=[int(x.shape[0]) for _, x in trace], trace_files=[], basis_files=sorted(os.listdir(d)),
                   basis_dir=d, saved=[(n, x) for n, x in saved])
        for old in os.listdir(HERE):
            if old.startswith("transport_uncond_small.trace"):
                os.remove(os.path.join(HERE, old))
        for i, r0 in enumerate(range(0, rows.shape[0], ROWS_PER_FILE)):
            fn = f"transport_uncond_small.trace{i}.pt"
            torch.save(rows[r0:r0 + ROWS_PER_FILE].clone(), os.path.join(HERE, fn))
            fix["trace_files"].append(fn)
        torch.save(fix, os.path.join(HERE, "transport_uncond_small.pt"))
        from collections import Counter
        print("unet calls", len(trace), "by batch", dict(Counter(fix["trace_batch"])), "h_t_idx", fix["h_t_idx"], "edit_t_idx", fix["edit_t_idx"])
        print("saved", [(n, tuple(x.shape)) for n, x in saved])
    finally:
        os.chdir(cwd)
    for f in sorted(os.listdir(HERE)):
        if f.startswith("transport_uncond_small"):
            print(f, os.path.getsize(os.path.join(HERE, f)))


if __name__ == "__main__":
    main()
