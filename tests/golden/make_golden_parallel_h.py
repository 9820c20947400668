"""Generate the parallel-h fixture by RUNNING THE REFERENCE'S OWN DRIVER (build container only):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_parallel_h.py

``EditUncondDiffusion.run_edit_global_frechet_mean_zt`` (src/modules/edit.py:951-1246) with edit_xt = 'parallel-h' and frechet_mean_space = 'h', in
the manner of make_golden_frechet.py and on its toy ``PullBackDDPM``, weights, scheduler, sample and PRE-PLACED bases (frechet_uncond_small.pt: the
global u basis and the sample's own local basis, so the reference takes its load branches).  The three regularisation switches are off (they name
methods the reference never defines).  Two runs: use_sega_reg False and True (sega_reg_sigma = 1.0), vis_num = 4, vis_num_pc = 1,
local_projection = True.

The reference hands ``inv_jac_xt`` the INDEX ``t=self.edit_t_idx`` where the U-Net takes a timestep.  The method is compiled from its own source with
that one argument replaced by the timestep ``self.scheduler.timesteps[self.edit_t_idx]`` (asserted to match exactly once); nothing else differs.

x_edit_step_size is picked here, on the reference's data alone, as the first of STEP_SIZES for which
  - the direction turns: cos(v_first, v_last) < 0.99 on at least one chain of the run without the SEGA rule, and
  - in the SEGA run every element of every v_k is at least 1e-4 (relative) away from its threshold sega_reg_sigma * std(v_k), so that no decision can
    flip under fp32 noise.

Fixture (every file below 1 MiB)
  parallel_h_uncond_small.pt            args (x_edit_step_size among them), edit_t_idx, the timestep used, and per run ("plain", "sega"): the (t, batch)
                                        of every U-Net call, the EXP_NAMEs, the plot names, per chain the inputs x_j and raw outputs of every
                                        inv_jac_xt call, the v_k as applied (after the rule) and the states
  parallel_h_uncond_small.saved.pt      per run, every tvu.save_image call (name, tensor) in order
  parallel_h_uncond_small.trace<i>.pt   the inputs of the U-Net calls of both runs (plain then sega), concatenated along the batch, 80 rows per file
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

import torch  # noqa: E402

from make_golden import import_reference  # noqa: E402

ROWS_PER_FILE = 80
T_ARG = "x=xt[-1], t=self.edit_t_idx, op=op, block_idx=block_idx,"
T_FIX = "x=xt[-1], t=self.scheduler.timesteps[self.edit_t_idx], op=op, block_idx=block_idx,"
# On this toy net the direction turns slowly: 1 - cos grows like the square of the size and is 0.005 at 64 (|x_t| is about 55), so the search starts
# where it passes 0.01.  Some 25 000 elements go through the rule in a run, so only about one size in three keeps them all 1e-4 away.
STEP_SIZES = tuple(float(s) for s in range(92, 200, 4))
SIGMA, MARGIN, TURN = 1.0, 1e-4, 0.99


def main():
    torch.set_num_threads(8)
    ru, rd = import_reference()
    import modules.edit as redit
    from diffusion_pullback_amd import configs as cf
    from oracle import unet_ddpm

    f = torch.load(os.path.join(HERE, "frechet_uncond_small.pt"), weights_only=False)
    a0 = f["args"]
    saved, plots = [], []
    redit.tvu.save_image = lambda x, path, **kw: saved.append((os.path.basename(path), x.detach().clone()))
    redit.tqdm = lambda it, **kw: it

    class Plt:
        scatter = legend = close = staticmethod(lambda *a, **k: None)
        savefig = staticmethod(lambda path, **k: plots.append(os.path.basename(path)))
    redit.plt = Plt
    src = textwrap.dedent(inspect.getsource(redit.EditUncondDiffusion.run_edit_global_frechet_mean_zt))
    assert src.count(T_ARG) == 1
    ns_run = {}
    exec(compile(src.replace(T_ARG, T_FIX), "<run_edit_global_frechet_mean_zt with the timestep handed to inv_jac_xt>", "exec"), redit.__dict__, ns_run)
    run = ns_run["run_edit_global_frechet_mean_zt"]

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
        trace, jac, quiet = [], [], [False]
        fwd0, ij0 = net.forward, net.inv_jac_xt

        def traced(x, t, *a, **k):
            if not quiet[0]:
                trace.append((float(t), x.detach().clone()))
            return fwd0(x, t, *a, **k)

        def traced_ij(x=None, t=None, **k):                   # (what inv_jac_xt itself runs through the net is not a U-Net call of the job)
            quiet[0] = True
            try:
                v = ij0(x=x, t=t, **k)
            finally:
                quiet[0] = False
            jac.append((float(t), x.detach().clone(), v.detach().clone()))
            return v

        class A:
            noise_schedule = None; device = "cpu"; dtype = torch.float32
        eu = object.__new__(redit.EditUncondDiffusion)
        eu.pca_device = eu.buffer_device = "cpu"; eu.memory_bound = 50; eu.device = "cpu"; eu.dtype = torch.float32; eu.seed = 0
        eu.save_result_as = "image"; eu.unet = net; eu.scheduler = ru.YHCustomScheduler(A()); eu.model_name = a0["model_name"]
        eu.image_size = 32; eu.c_in = 3; eu.dataset = {0: f["x0"]}; eu.dataset_name = a0["dataset_name"]
        eu.for_steps, eu.inv_steps, eu.use_yh_custom_scheduler, eu.edit_t, eu.h_t = a0["for_steps"], a0["inv_steps"], True, a0["edit_t"], a0["h_t"]
        eu.scheduler.set_timesteps(eu.for_steps, device="cpu")
        eu.edit_t_idx = (eu.scheduler.timesteps - eu.edit_t * 1000).abs().argmin()
        eu.h_t_idx = (eu.scheduler.timesteps - eu.h_t * 1000).abs().argmin()
        assert int(eu.edit_t_idx) == f["edit_t_idx"]
        eu.performance_boosting_t_idx = 1000                   # eta = 1 tail off: its noise is a device RNG draw, not reproducible
        eu.use_x_space_guidance = True; eu.edit_xt = "parallel-h"; eu.edit_ht = "default"; eu.scheduler_name = a0["scheduler_name"]
        eu.frechet_mean_space = "h"
        eu.use_dynamic_thresholding = eu.use_preserve_contrast = eu.use_preserve_norm = False
        eu.x_space_guidance_edit_step, eu.x_space_guidance_scale, eu.x_space_guidance_num_step = 1.0, 0.1, 8
        eu.result_folder, eu.obs_folder = "res", "obs"
        os.makedirs(f["dirs"]["own"], exist_ok=True); os.makedirs(f["dirs"]["glob"], exist_ok=True)
        torch.save(f["own_u"], os.path.join(f["dirs"]["own"], "u-xt-CelebA_HQ_0-0.8T-mid-block_0-seed_0.pt"))
        torch.save(f["own_vT"], os.path.join(f["dirs"]["own"], "vT-xt-CelebA_HQ_0-0.8T-mid-block_0-seed_0.pt"))
        torch.save(f["global_u"], os.path.join(f["dirs"]["glob"], "u-0.8T-mid-block_0-seed_0-num_local_basis_4.pt"))
        net.forward, net.inv_jac_xt = traced, traced_ij
        vis_num = a0["vis_num"]
        kw = dict(idx=0, op="mid", block_idx=0, vis_num=vis_num, pca_rank=a0["pca_rank"], num_local_basis=a0["num_local_basis"], local_projection=True,
                  vis_num_pc=1, vis_pc_list=None)

        def one_run(step_size, sega):
            saved.clear(); plots.clear(); trace.clear(); jac.clear()
            eu.x_edit_step_size, eu.use_sega_reg, eu.sega_reg_sigma = step_size, sega, SIGMA
            with contextlib.redirect_stdout(io.StringIO()):
                run(eu, **kw)
            names = [n[len("x0_gen-"):-len(".png")] for n, _ in saved if n.startswith("x0_gen-xt-")]
            assert len(names) == 2 and len(jac) == 2 * vis_num, (names, len(jac))
            decode = [x for t, x in trace if x.shape[0] == vis_num + 1]
            per = len(decode) // 2
            chains, margin = [], float("inf")
            for c in range(2):
                calls = jac[c * vis_num:(c + 1) * vis_num]
                states = decode[c * per]                                                # the chain's first decode call holds its vis_num + 1 states
                assert all(torch.equal(calls[j][1][0], states[j]) for j in range(vis_num))
                raw = torch.stack([v.reshape(-1) for _, _, v in calls])
                vk = raw.clone()
                if sega:                                                                # edit.py:1212-1214, restated to measure the margin
                    thr = torch.stack([SIGMA * v.std() for _, _, v in calls])[:, None]
                    margin = min(margin, float(((raw.abs() - thr).abs() / thr).min()))
                    vk = raw.masked_fill(raw.abs() < thr, 0.0)
                each = step_size / vis_num
                for j in range(vis_num):                                                # edit.py:1216: the states are those v_k, bit for bit
                    assert torch.equal(states[j + 1], states[j] + vk[j].reshape(states[j].shape) * each), (c, j)
                chains.append(dict(t=[t for t, _, _ in calls], x=torch.stack([x[0] for _, x, _ in calls]), v_raw=raw, vk=vk, states=states.clone()))
            turn = min(float(torch.nn.functional.cosine_similarity(c["v_raw"][0], c["v_raw"][-1], dim=0)) for c in chains)
            return dict(trace_t=[t for t, _ in trace], trace_batch=[int(x.shape[0]) for _, x in trace], trace_x=[x for _, x in trace],
                        saved=[(n, x) for n, x in saved], plots=list(plots), names=names, chains=chains), turn, margin

        for step_size in STEP_SIZES:
            plain, turn, _ = one_run(step_size, False)
            for n, _ in plain["saved"]:
                assert not os.path.exists(os.path.join("res", n))
            sega, _, margin = one_run(step_size, True)
            print(f"x_edit_step_size {step_size}: cos(v_first, v_last) {turn:.4f}, SEGA margin {margin:.2e}")
            if turn < TURN and margin >= MARGIN:
                break
        else:
            raise SystemExit("no step size of STEP_SIZES turns the direction and keeps the SEGA margin")
        assert turn < TURN and margin >= MARGIN
        runs = dict(plain=plain, sega=sega)
        rows = torch.cat([x for r in ("plain", "sega") for x in runs[r].pop("trace_x")], dim=0)
        args = dict(a0, x_edit_step_size=step_size, sega_reg_sigma=SIGMA, vis_num_pc=1, turn=turn, sega_margin=margin, runs=None)
        fix = dict(args=args, edit_t_idx=int(eu.edit_t_idx), edit_t=float(eu.scheduler.timesteps[eu.edit_t_idx]), runs=runs, trace_files=[])
        for old in os.listdir(HERE):
            if old.startswith("parallel_h_uncond_small.trace"):
                os.remove(os.path.join(HERE, old))
        for i, r0 in enumerate(range(0, rows.shape[0], ROWS_PER_FILE)):
            fn = f"parallel_h_uncond_small.trace{i}.pt"
            torch.save(rows[r0:r0 + ROWS_PER_FILE].clone(), os.path.join(HERE, fn))
            fix["trace_files"].append(fn)
        torch.save({r: runs[r].pop("saved") for r in ("plain", "sega")}, os.path.join(HERE, "parallel_h_uncond_small.saved.pt"))
        torch.save(fix, os.path.join(HERE, "parallel_h_uncond_small.pt"))
        for r in ("plain", "sega"):
            print(r, "unet calls", len(runs[r]["trace_t"]), "rows", sum(runs[r]["trace_batch"]), "names", runs[r]["names"], "plots", runs[r]["plots"],
                  "kept", [[int((v != 0).sum()) for v in c["vk"]] for c in runs[r]["chains"]])
    finally:
        os.chdir(cwd)
    for fn in sorted(os.listdir(HERE)):
        if fn.startswith("parallel_h_uncond_small"):
            print(fn, os.path.getsize(os.path.join(HERE, fn)))


if __name__ == "__main__":
    main()
