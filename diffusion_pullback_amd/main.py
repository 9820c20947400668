"""Command line of the pullback editing path -- ``python -m diffusion_pullback_amd.main --flags``.

Keeps the reference's live-path flags and preset rules so its scripts run unchanged
(reference src/main.py:13-34, src/utils/define_argparser.py:15-242, src/scripts/*.sh):
``--run_edit_local_encoder_pullback_zt True`` dispatches to ``EditStableDiffusion`` when
``'stable-diffusion' in model_name`` and to ``EditUncondDiffusion`` otherwise, with the call-site
constants of main.py:30-34 (op='mid', block_idx=0, vis_num=4, vis_num_pc=2, pca_rank=2) as defaults.
Flags of the reference's dead experiments are accepted and ignored with a note.
New flags (not in the reference): --pca_rank, --op, --block_idx, --dtype bf16, --weights (state-dict
file; default: seeded synthetic weights, there are no checkpoints offline), --net_scale (reduced nets),
--vae (none | synthetic | <state-dict file>: decode the edited latents to PNGs with the on-device AutoencoderKL),
--text_encoder (none | synthetic | <state-dict file>) + --tokenizer_dir (CLIP vocab.json / merges.txt): on-device prompt encoder.
``--run_sample_encoder_local_tangent_space_zt True`` (reference src/main.py:45-91) samples the local tangent spaces of --num_local_basis latents at
every timestep of --h_t_list (comma-separated; default: the single --h_t), with --fix_xt / --fix_t for the unconditional net; the pending
(latent, h_t) pairs advance together, each at its own timestep.  The reference's call sites fix pca_rank=50 and loop over its EDIT_T_LIST (and, for
SD, over MS-COCO captions, which are not available offline): here --pca_rank, --h_t_list and --edit_prompt say the same.
``--run_tangent_space_distance True --distance_space x|h`` computes what those files are saved for: the principal angles and the geodesic
distance ||theta||_2 between every two sampled tangent spaces (x: the spans of vT, h: the spans of u), on the GPU (geometry.py).  It honours --h_t_list,
--num_local_basis, --pca_rank, --op, --block_idx, --edit_prompt, --fix_xt and --fix_t exactly as the sampling job does, reads that job's files (a missing
one is an error: nothing is sampled silently) and writes tangent_space_distance-<space>-....pt and .png next to them.  Distances only: no means.
``--run_tangent_space_clusters True --num_clusters C --cluster_rank r`` clusters the same files into C families by flag k-means, each with a rank-r flag
mean as its centre (geometry.flag_kmeans; --cluster_rank 0, the default, means --pca_rank).  It takes --distance_space and the sampling job's flags as
the distance job does, runs after the sampling job, and writes tangent_space_clusters-<space>-C<C>-r<r>-....pt (labels, centres, affinity, ...) and .png.
``--run_tangent_space_pga True --pga_base frechet|flag --pga_modes M`` describes how the same files vary around their centre: principal geodesic
analysis of their log maps at the Frechet (or flag) mean (geometry.grassmann_pga; --pga_modes 0, the default, means min(pairs - 1, 16)), and, when
--h_t_list holds more than one timestep, the tangent-space regression on h_t (r2, slope_norm).  It takes --distance_space and the sampling job's flags as
the distance job does, runs after the sampling job, and writes tangent_space_pga-<space>-<base>-M<M>-....pt (base, modes, variance, scores, ...), a scree
plot and a scatter of the first two scores coloured by h_t.
``--run_edit_parallel_transport True --sample_idx_0 i --sample_idx_1 j`` (the reference's flags, define_argparser.py:117-119; unconditional nets only, with
--is_stable_diffusion models it is an error) edits sample j along the principal directions of sample i carried over by parallel transport between their
local tangent spaces at --h_t, and sample i along its own, at --edit_t; --sample_idx_1_list 1,2,3 (new) serves several targets in one call.  It honours
--op, --block_idx, --pca_rank (the reference's call site fixes 50), --vis_num, --vis_num_pc and --trajectory_batch, reads the u- / vT- files of the sampling job when they are there and
computes the missing ones together.
``--run_edit_global_frechet_mean_zt True --frechet_mean_space x|h --num_local_basis n`` (the reference's flags, define_argparser.py:112-113; unconditional
nets only) edits --sample_idx along the rows of a global basis: the Frechet mean on the Grassmannian of the n local tangent spaces of the 'Random'
sampling directory at --h_t (x: the spans of vT, h: the spans of u; missing ones are sampled together), computed on the GPU (geometry.frechet_mean,
--frechet_max_iter, --frechet_tol: both new; the reference hands the problem to pymanopt) and cached as v- / u-....pt with an info- file beside it.
--local_projection False (space x only) skips the projection on the sample's own tangent space.  It honours --op, --block_idx, --pca_rank,
--vis_num, --vis_num_pc and --trajectory_batch as the transport job does.
--frechet_init member|flag (new; default member: local basis 0) starts the iteration at the flag mean of the local bases instead.
``--run_edit_global_flag_mean_zt True --flag_mean_space x|h --flag_rank r`` (new; unconditional nets only) edits --sample_idx along the rows of the
flag (extrinsic) mean of the same local bases: the top r eigenvectors of their mean projector (geometry.flag_mean; --flag_rank 0, the default, means
--pca_rank), cached as v- / u-...-rank_<r>.pt with an info- file that holds the spectrum.  It takes the Frechet job's other flags.
--flag_mean_kind mean|median (new; default mean) makes that basis the flag median of the local bases instead (geometry.flag_median: the L1
counterpart, by iteratively reweighted flag means; --flag_median_eps, the clamp of the weights, and --flag_median_max_rounds), cached under the same
names with -median appended; its info- file also ranks the local bases from typical to outlying (member_weight, distance).
``--run_edit_global_hungarian_mean_zt True --hungarian_mean_space x|h`` (the reference's flags, define_argparser.py:121-122; unconditional nets only)
edits --sample_idx along the other global basis: the Hungarian-matched mean of the same local bases -- the directions of every basis matched one to
one and sign by sign to those of basis 0 and averaged (geometry.hungarian_mean; --hungarian_distance 1/cosine|cosine and --hungarian_max_sweeps are
new).  Both bases are computed and cached, u-....pt from the u's and v-....pt from the vT's, each with an info- file; x edits along v, h along u.
``--edit_xt parallel-x|parallel-h`` (the reference's flag, define_argparser.py:52) says how the three global-basis jobs move x_t.  parallel-x, the
default, is the x-space guidance above: one x-space direction computed at x_t, pushed along at every step.  parallel-h (space h only; unconditional
nets only) holds the h-space direction u_pc fixed instead and recomputes the x-space direction at every state: --vis_num steps
x <- x + (--x_edit_step_size / vis_num) * inv_jac_xt(x, t, u_pc), all chains advanced together on the device (PullbackUNet.inv_jac_chain), then the same
decode into the same picture names; --use_sega_reg True --sega_reg_sigma s zeroes the elements of each direction below s standard deviations
(edit.py:1212-1214).  --local_projection False is allowed there and needs no local basis at all.  Every chain leaves chain-<name>.pt in the obs
folder: ||J^T u||, the h-space shift along u and |h - h0| per step.  Deviations: t is the timestep (the reference passes the index edit_t_idx);
the reference's dynamic_thresholding / preserve_norm / preserve_contrast are methods it never defines and are not built.
``--edit_xt newton-h`` (new; space h only; unconditional nets only) is the third value: every (pc, +-) chain starts at x_t and aims at the h-space
shift --h_edit_step_size along +-u_pc in --vis_num damped Gauss-Newton steps, each the least-squares inverse of the Jacobian applied to the remaining
residual by --newton_iters CGLS iterations (PullbackUNet.newton_h_chain; --newton_damping, the relative Tikhonov term, and --newton_radius, the clamp
of a step's length in x, 0 = off), where parallel-h takes the steepest-descent direction.  Same picture names, skip rule and --local_projection False
allowance as parallel-h; a pos chain moves h ALONG u_pc (parallel-h: against).  Every chain leaves newton-<name>.pt in the obs folder.
``--edit_ht default|h_space_guidance`` (the reference's flag, define_argparser.py:53) is the third way: with --edit_xt at its default and space h
(unconditional nets only), every (pc, +-) experiment runs --vis_num chains from x_t whose h-space direction u_pc is ADDED at the tap at every DDIM step
from --edit_t down to --no_edit_t (default 0.5), with the scales +-linspace(0, --h_edit_step_size, vis_num); --h_guidance_mode asyrp (default: the
shift enters the predicted x0 only, Kwon et al.'s asymmetric process) or symmetric (the plain DDIM step of the shifted net).  The chains run on the
device (PullbackUNet.h_space_guidance), then the plain decode from no_edit_t into the same picture names; --local_projection False is allowed as for
parallel-h.  Every experiment leaves hguide-<name>.pt in the obs folder: ||e_s - e|| and the distance from the plain step per chain and step, the
scales, the timesteps and the latents at no_edit_t.  The reference calls a h_space_guidance method it never defines; DESIGN.md states what is built.
``--run_geodesic_interpolation True --sample_idx_0 i --sample_idx_1 j --geodesic_points m --geodesic_lambda l --geodesic_max_iter n --geodesic_tol tol``
(both drivers; with --h_t --op --block_idx) joins the latents of two samples at h_t by the shortest path under the pullback metric of get_h
(PullbackUNet.pullback_geodesic, m interior points, started from slerp), measures lerp, slerp and the geodesic alike (energy, h-length, uniformity) and
decodes the three curves: x0_gen-Geodesic-<dataset>_<i>_<j>-<h_t>T-<op>-block_<b>-{lerp|slerp|geodesic}.png and geodesic-Geodesic-<...>.pt.
"""
from __future__ import annotations

import argparse
import os
import random
import sys

import numpy as np
import torch

from . import configs as cf
from .edit import EditStableDiffusion, EditUncondDiffusion
from .pullback import PullbackUNet

# reference src/configs/params.py:1-27
X_SPACE_GUIDANCE_SCALE_DICT = {
    "stable-diffusion": {1.0: 0.5, 0.9: 0.5, 0.8: 1, 0.7: 1, 0.6: 2, 0.5: 2, 0.4: 2, 0.3: 2, 0.2: 2, 0.1: 2, 0.0: 0},
    "uncond": {1.0: 0.5, 0.8: 1, 0.6: 4, 0.4: 16, 0.2: 16},
}


def str2bool(v):
    if isinstance(v, bool):
        return v
    if v.lower() in ("true",):
        return True
    if v.lower() in ("false",):
        return False
    raise argparse.ArgumentTypeError("Boolean value expected.")


_FLAGS = [  # (name, type, default) -- define_argparser.py:20-110, live path only
    ("sh_file_name", str, ""), ("device", str, "cuda:0"), ("dtype", str, "fp32"), ("seed", int, 0), ("result_folder", str, "./runs/"),
    ("model_name", str, ""), ("dataset_name", str, ""), ("image_size", int, 256), ("c_in", int, 3), ("sample_idx", int, 0),
    ("for_prompt", str, ""), ("inv_prompt", str, ""), ("neg_prompt", str, ""), ("for_steps", int, 100), ("inv_steps", int, 100),
    ("performance_boosting_t", float, 0.0), ("use_yh_custom_scheduler", str2bool, True), ("guidance_scale", float, 0),
    ("edit_prompt", str, ""), ("use_x_space_guidance", str2bool, False), ("x_space_guidance_edit_step", float, 1),
    ("x_space_guidance_scale", float, 0), ("x_space_guidance_num_step", int, 0), ("x_space_guidance_use_edit_prompt", str2bool, True),
    ("h_t", float, 0.8), ("edit_t", float, 1.0), ("x_edit_step_size", float, 0), ("pca_device", str, "cpu"), ("buffer_device", str, "cpu"),
    ("save_result_as", str, "image"), ("run_ddim_forward", str2bool, False), ("run_ddim_inversion", str2bool, False),
    ("run_edit_local_encoder_pullback_zt", str2bool, False),
    # define_argparser.py: the tangent-space sampling job of main.py:45-91 (h_t_list is new: the reference edits EDIT_T_LIST in its source)
    ("run_sample_encoder_local_tangent_space_zt", str2bool, False), ("num_local_basis", int, 10), ("h_t_list", str, ""),
    ("fix_xt", str2bool, False), ("fix_t", str2bool, False),
    # new: principal angles / geodesic distances between the sampled tangent spaces (geometry.py); x = the spans of vT, h = the spans of u
    ("run_tangent_space_distance", str2bool, False),
    # new: flag k-means of the sampled tangent spaces (geometry.flag_kmeans); cluster_rank 0: pca_rank
    ("run_tangent_space_clusters", str2bool, False), ("num_clusters", int, 2), ("cluster_rank", int, 0),
    # new: principal geodesic analysis of the sampled tangent spaces (geometry.grassmann_pga); pga_modes 0: the default of grassmann_pga
    ("run_tangent_space_pga", str2bool, False), ("pga_base", str, "frechet"), ("pga_modes", int, 0),
    # define_argparser.py:117-119: the parallel-transport edit job (unconditional nets); sample_idx_1_list is new: several targets in one call
    ("run_edit_parallel_transport", str2bool, False), ("sample_idx_0", int, 0), ("sample_idx_1", int, 0), ("sample_idx_1_list", str, ""),
    # define_argparser.py:112-114: the global-basis edit job (unconditional nets).  local_projection defaults to True here, the default of the method
    # (the reference's flag defaults to False, with which its h-space branch leaves vk undefined); frechet_max_iter / frechet_tol are new (the
    # reference hands pymanopt 10 000 iterations)
    ("run_edit_global_frechet_mean_zt", str2bool, False), ("frechet_mean_space", str, "x"), ("frechet_max_iter", int, 1000),
    ("frechet_tol", float, 1e-6), ("local_projection", str2bool, True),
    # new: the start of the Karcher iteration (member: local basis 0; flag: the flag mean), and the flag-mean global-basis job (flag_rank 0: pca_rank)
    ("frechet_init", str, "member"), ("run_edit_global_flag_mean_zt", str2bool, False), ("flag_mean_space", str, "x"), ("flag_rank", int, 0),
    # new: the flag-mean job's basis as the flag median (geometry.flag_median: iteratively reweighted flag means), its clamp and its round limit
    ("flag_mean_kind", str, "mean"), ("flag_median_eps", float, 1e-5), ("flag_median_max_rounds", int, 50),
    # define_argparser.py:121-122: the other global-basis job (unconditional nets); hungarian_mean_space defaults to x, what the reference's method
    # does (its flag has no consumer); hungarian_distance / hungarian_max_sweeps are new (the reference passes distance='1/cosine')
    ("run_edit_global_hungarian_mean_zt", str2bool, False), ("hungarian_mean_space", str, "x"), ("hungarian_distance", str, "1/cosine"),
    ("hungarian_max_sweeps", int, 20),
    # define_argparser.py:52, :84: how the global-basis jobs move x_t.  parallel-x (default): x-space guidance along one direction fixed at x_t;
    # parallel-h: the h-space direction held fixed, the x-space direction recomputed at every one of vis_num steps of x_edit_step_size / vis_num
    # (edit.py:1202-1229), with the SEGA rule of edit.py:1212-1214 under --use_sega_reg (sega_reg_sigma 1.0: the reference's commented default)
    ("edit_xt", str, "parallel-x"), ("use_sega_reg", str2bool, False), ("sega_reg_sigma", float, 1.0),
    # new: --edit_xt newton-h, the third value: every chain aims at the h-space shift h_edit_step_size along u_pc in vis_num damped Gauss-Newton steps
    # of newton_iters CGLS iterations each (PullbackUNet.newton_h_chain); newton_damping: the relative Tikhonov term; newton_radius: the clamp of a
    # step's length in x (0: off)
    ("newton_iters", int, 8), ("newton_damping", float, 0.1), ("newton_radius", float, 0.0),
    # define_argparser.py:53, :82-83: the third branch of the global-basis jobs.  h_space_guidance (with edit_xt at its default): the h-space direction
    # is added at the tap at every DDIM step from edit_t down to no_edit_t (edit.py:1232-1245), with scales up to h_edit_step_size; h_guidance_mode
    # is new: asyrp (the shift enters the predicted x0 only) or symmetric (the plain DDIM step of the shifted net)
    ("edit_ht", str, "default"), ("h_edit_step_size", float, 0), ("no_edit_t", float, 0.5), ("h_guidance_mode", str, "asyrp"),
    # new: the pullback geodesic between the latents of --sample_idx_0 and --sample_idx_1 at --h_t (PullbackUNet.pullback_geodesic), against lerp and slerp
    ("run_geodesic_interpolation", str2bool, False), ("geodesic_points", int, 8), ("geodesic_lambda", float, 0.0), ("geodesic_max_iter", int, 200),
    ("geodesic_tol", float, 1e-4),
    # new
    ("pca_rank", int, 2), ("op", str, "mid"), ("block_idx", int, 0), ("vis_num", int, 4), ("vis_num_pc", int, 2), ("weights", str, ""),
    ("net_scale", str, "full"), ("vae", str, "none"), ("text_encoder", str, "none"), ("tokenizer_dir", str, ""),
    ("timing", str2bool, False),      # wall-clock breakdown of the run by phase (timing.py; synchronises at phase boundaries)
    # U-Net batch of the edit trajectories: the 2 * vis_num_pc independent (pc, +-) edits of edit.py:276-307 run together (x-space guidance as one batch-2n call per
    # step, the n * (vis_num + 1) decode trajectories as one batch).  Same files, tensors equal up to 16-bit rounding (tile / split-K choices depend on the batch);
    # 0 / 1 = one experiment after another, memory_bound latents per call (the setting for bitwise-reproducible runs); an explicit --memory_bound caps it
    # (and replaces the per-model memory_bound constant: it is then the bound of every U-Net call, the 2 of an x-space-guidance pair being the floor)
    ("trajectory_batch", int, 20),
]


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    for name, typ, default in _FLAGS:
        p.add_argument("--" + name, type=typ, default=default, required=False)
    p.add_argument("--note", type=str, required=True)
    # --memory_bound is NOT a flag of the reference (define_argparser.py:211-221 sets memory_bound to a per-model constant, kept in preset()); here an explicit
    # value is the user's bound on the U-Net batch -- decode chunks, trajectory batching, the guidance chains per call and the engine's max_batch all respect it
    p.add_argument("--memory_bound", type=int, default=None)
    p.add_argument("--distance_space", type=str, default="x", choices=["x", "h"])
    args, extra = p.parse_known_args(argv)
    if args.memory_bound is not None and args.memory_bound < 1:
        p.error("--memory_bound must be a positive integer")
    args.memory_bound_given = args.memory_bound
    try:
        args.h_t_values = [float(v) for v in args.h_t_list.split(",") if v.strip()] or [args.h_t]
    except ValueError:
        p.error("--h_t_list must be comma-separated numbers, e.g. 0.8,0.5")
    if args.fix_xt and args.fix_t:
        p.error("--fix_xt and --fix_t exclude each other")
    try:
        args.sample_idx_1_values = [int(v) for v in args.sample_idx_1_list.split(",") if v.strip()] or [args.sample_idx_1]
    except ValueError:
        p.error("--sample_idx_1_list must be comma-separated integers, e.g. 1,2,3")
    if args.run_edit_parallel_transport and "stable-diffusion" in args.model_name:
        p.error("--run_edit_parallel_transport is a job of the unconditional nets only: the reference has no Stable Diffusion parallel transport "
                "(its run_edit_parallel_transport belongs to EditUncondDiffusion)")
    if args.run_edit_global_frechet_mean_zt and "stable-diffusion" in args.model_name:
        p.error("--run_edit_global_frechet_mean_zt is a job of the unconditional nets only: the reference has no Stable Diffusion global Frechet basis "
                "(its run_edit_global_frechet_mean_zt belongs to EditUncondDiffusion)")
    if args.run_edit_global_frechet_mean_zt and args.frechet_mean_space not in ("x", "h"):
        p.error("--frechet_mean_space must be x (the spans of vT) or h (the spans of u)")
    if args.run_edit_global_frechet_mean_zt and args.frechet_mean_space == "h" and not args.local_projection and args.edit_xt not in ("parallel-h", "newton-h") and args.edit_ht != "h_space_guidance":
        p.error("--local_projection False is valid for --frechet_mean_space x only")
    if args.frechet_init not in ("member", "flag"):
        p.error("--frechet_init must be member (start at local basis 0) or flag (start at the flag mean of the local bases)")
    if args.run_edit_global_flag_mean_zt and "stable-diffusion" in args.model_name:
        p.error("--run_edit_global_flag_mean_zt is a job of the unconditional nets only: the reference has no Stable Diffusion global basis "
                "(its global-basis jobs belong to EditUncondDiffusion)")
    if args.run_edit_global_flag_mean_zt and args.flag_mean_space not in ("x", "h"):
        p.error("--flag_mean_space must be x (the spans of vT) or h (the spans of u)")
    if args.run_edit_global_flag_mean_zt and args.flag_mean_space == "h" and not args.local_projection and args.edit_xt not in ("parallel-h", "newton-h") and args.edit_ht != "h_space_guidance":
        p.error("--local_projection False is valid for --flag_mean_space x only")
    if args.run_edit_global_flag_mean_zt and not 0 <= args.flag_rank <= args.pca_rank:
        p.error("--flag_rank must lie in [1, --pca_rank] (0: --pca_rank)")
    if args.flag_mean_kind != "mean" and "stable-diffusion" in args.model_name:
        p.error("--flag_mean_kind belongs to --run_edit_global_flag_mean_zt, a job of the unconditional nets only: the reference has no Stable "
                "Diffusion global basis")
    if args.flag_mean_kind not in ("mean", "median"):
        p.error("--flag_mean_kind must be mean (the flag mean of the local bases) or median (their flag median)")
    if not args.flag_median_eps > 0 or args.flag_median_max_rounds < 0:
        p.error("--flag_median_eps must be positive and --flag_median_max_rounds >= 0")
    if args.run_edit_global_hungarian_mean_zt and "stable-diffusion" in args.model_name:
        p.error("--run_edit_global_hungarian_mean_zt is a job of the unconditional nets only: the reference has no Stable Diffusion global Hungarian "
                "basis (its run_edit_global_hungarian_mean_zt belongs to EditUncondDiffusion)")
    if args.run_edit_global_hungarian_mean_zt and args.hungarian_mean_space not in ("x", "h"):
        p.error("--hungarian_mean_space must be x (the directions of vT) or h (the directions of u)")
    if args.run_edit_global_hungarian_mean_zt and args.hungarian_mean_space == "h" and not args.local_projection and args.edit_xt not in ("parallel-h", "newton-h") and args.edit_ht != "h_space_guidance":
        p.error("--local_projection False is valid for --hungarian_mean_space x only")
    if args.run_edit_global_hungarian_mean_zt and args.hungarian_distance not in ("1/cosine", "cosine"):
        p.error("--hungarian_distance must be 1/cosine (the reference's call) or cosine")
    if args.run_edit_global_hungarian_mean_zt and args.hungarian_max_sweeps < 1:
        p.error("--hungarian_max_sweeps must be >= 1")
    if args.edit_xt not in ("parallel-x", "parallel-h", "newton-h"):
        p.error("--edit_xt must be parallel-x (x-space guidance along a direction fixed at x_t), parallel-h (the h-space direction held fixed) or "
                "newton-h (damped Gauss-Newton steps towards an h-space shift)")
    if args.edit_xt == "parallel-h" and not args.x_edit_step_size > 0:
        p.error("--edit_xt parallel-h needs --x_edit_step_size > 0: the chain takes --vis_num steps of x_edit_step_size / vis_num")
    if args.edit_xt == "parallel-h" and "stable-diffusion" in args.model_name:
        p.error("--edit_xt parallel-h belongs to the global-basis jobs of the unconditional nets: the reference's Stable Diffusion driver has no such "
                "branch")
    if args.edit_xt == "newton-h":
        if "stable-diffusion" in args.model_name:
            p.error("--edit_xt newton-h belongs to the global-basis jobs of the unconditional nets, as parallel-h: the Stable Diffusion driver has no "
                    "such branch")
        if args.h_edit_step_size == 0:
            p.error("--edit_xt newton-h needs --h_edit_step_size != 0: the h-space shift the chain aims at")
        if args.edit_ht == "h_space_guidance":
            p.error("--edit_xt newton-h and --edit_ht h_space_guidance exclude each other: the guidance branch runs with --edit_xt at its default")
        if args.newton_iters < 0 or not args.newton_damping >= 0 or not args.newton_radius >= 0:
            p.error("--newton_iters, --newton_damping and --newton_radius must not be negative (--newton_radius 0: no clamp)")
        for job, space in (("run_edit_global_frechet_mean_zt", "frechet_mean_space"), ("run_edit_global_flag_mean_zt", "flag_mean_space"),
                           ("run_edit_global_hungarian_mean_zt", "hungarian_mean_space")):
            if getattr(args, job) and getattr(args, space) != "h":
                p.error(f"--edit_xt newton-h aims at an h-space shift: --{space} must be h")
    if args.edit_ht not in ("default", "h_space_guidance"):
        p.error("--edit_ht must be default or h_space_guidance (the h-space direction added at the tap at every DDIM step from edit_t to no_edit_t)")
    if args.h_guidance_mode not in ("asyrp", "symmetric"):
        p.error("--h_guidance_mode must be asyrp (the shift enters the predicted x0 only) or symmetric (the plain DDIM step of the shifted net)")
    if args.edit_ht == "h_space_guidance":
        if "stable-diffusion" in args.model_name:
            p.error("--edit_ht h_space_guidance belongs to the global-basis jobs of the unconditional nets: the reference's Stable Diffusion driver has "
                    "no such branch")
        if args.edit_xt == "parallel-h":
            p.error("--edit_ht h_space_guidance and --edit_xt parallel-h exclude each other: the guidance branch runs with --edit_xt at its default")
        if args.h_edit_step_size == 0:
            p.error("--edit_ht h_space_guidance needs --h_edit_step_size != 0: the largest scale of the ladder of shifts")
        if not args.no_edit_t < args.edit_t:
            p.error("--edit_ht h_space_guidance needs --no_edit_t < --edit_t: the guided interval runs from edit_t down to no_edit_t")
        if args.performance_boosting_t > 0 and args.no_edit_t < args.performance_boosting_t:
            p.error("--edit_ht h_space_guidance: the guided interval must end at or above --performance_boosting_t (the decode takes eta = 1 below "
                    "it, the chain is eta = 0 only)")
        for job, space in (("run_edit_global_frechet_mean_zt", "frechet_mean_space"), ("run_edit_global_flag_mean_zt", "flag_mean_space"),
                           ("run_edit_global_hungarian_mean_zt", "hungarian_mean_space")):
            if getattr(args, job) and getattr(args, space) != "h":
                p.error(f"--edit_ht h_space_guidance adds an h-space direction at the tap: --{space} must be h")
    if args.run_tangent_space_clusters:
        pairs = max(0, args.num_local_basis) * len(args.h_t_values)
        if not 1 <= args.num_clusters <= pairs:
            p.error(f"--num_clusters must lie in [1, {pairs}], the number of (basis, h_t) pairs of --num_local_basis and --h_t_list")
        if not 0 <= args.cluster_rank <= args.pca_rank:
            p.error("--cluster_rank must lie in [1, --pca_rank] (0: --pca_rank)")
    if args.run_tangent_space_pga:
        pairs = max(0, args.num_local_basis) * len(args.h_t_values)
        if args.pga_base not in ("frechet", "flag"):
            p.error("--pga_base must be frechet (the Karcher mean) or flag (the flag mean)")
        if pairs < 2 or not 0 <= args.pga_modes <= min(64, pairs - 1):
            p.error(f"--pga_modes must lie in [1, {min(64, pairs - 1)}] (0: the default), one less than the (basis, h_t) pairs of --num_local_basis and --h_t_list")
    if args.run_geodesic_interpolation:
        if args.geodesic_points < 1:
            p.error("--geodesic_points must be >= 1: the points of the curve between its two ends")
        if not (0 <= args.geodesic_lambda < float("inf")):
            p.error("--geodesic_lambda must be finite and >= 0 (0: the pullback energy alone)")
        if args.geodesic_max_iter < 1 or not (0 <= args.geodesic_tol < float("inf")):
            p.error("--geodesic_max_iter must be >= 1 and --geodesic_tol finite and >= 0")
        if args.sample_idx_0 == args.sample_idx_1:
            p.error("--run_geodesic_interpolation joins two different samples: --sample_idx_0 and --sample_idx_1 are equal")
    if extra:
        print(f"note: ignoring flags of experiments outside the pullback path: {extra}")
    return args


def seed_everything(seed: int):
    os.environ["PYTHONHASHSEED"] = str(seed)
    np.random.seed(seed)
    random.seed(seed)
    torch.manual_seed(seed)


def preset(args):
    """define_argparser.py:145-233 (folders, derived args, asserts)."""
    seed_everything(args.seed)
    args.is_stable_diffusion = "stable-diffusion" in args.model_name
    if args.is_stable_diffusion:
        args.exp = f"Stable_Diffusion-{args.dataset_name}-{args.note}"
    else:
        # define_argparser.py:163-172.  The guided-diffusion names (:165-168) stop the reference with "please download the weight"; here they select
        # the ADM presets (configs.ADM_MODEL_NAMES) and run on --weights <state dict of the reference's UNetModel> or on synthetic weights
        if args.model_name not in ("CelebA_HQ_HF", "LSUN_church_HF", "FFHQ_HF") and args.model_name not in cf.ADM_MODEL_NAMES:
            raise ValueError("model_name choice: [CelebA_HQ_HF, LSUN_church_HF, FFHQ_HF, " + ", ".join(cf.ADM_MODEL_NAMES) + "]")
        args.exp = f"{args.model_name}-{args.dataset_name}-{args.note}"
    args.exp_folder = os.path.join(args.result_folder, args.exp)
    args.obs_folder = os.path.join(args.exp_folder, "obs")
    args.result_folder = os.path.join(args.exp_folder, "results")
    os.makedirs(args.obs_folder, exist_ok=True)
    os.makedirs(args.result_folder, exist_ok=True)
    args.device = torch.device(args.device)
    args.compute_dtype = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}.get(args.dtype)   # define_argparser.py:196 (+ bf16)
    if args.compute_dtype is None:
        raise ValueError("dtype choice: [fp32, fp16, bf16]")
    args.dtype = torch.float32                      # boundary dtype of latents
    if args.use_x_space_guidance:
        args.x_space_guidance_scale = X_SPACE_GUIDANCE_SCALE_DICT["stable-diffusion" if args.is_stable_diffusion else "uncond"][args.h_t]
    given = getattr(args, "memory_bound_given", None)
    if given:
        args.trajectory_batch = min(args.trajectory_batch, given)
    if args.is_stable_diffusion:
        args.c_in, args.image_size, args.memory_bound = 4, 64, given or 5
        assert args.use_yh_custom_scheduler
        assert args.performance_boosting_t <= 0
    else:
        args.c_in, args.image_size, args.memory_bound, args.noise_schedule = 3, 256, given or 50, "linear"
        assert args.use_yh_custom_scheduler
        assert args.for_steps == 100
        assert args.performance_boosting_t == 0.2
    return args


# tangents advanced together by the tangent-space job: 2 samples at pca_rank 50, 10 at 10.  The workspace grows with them.  Computed, not measured
# (dpb_engine_workspace_bytes of the whole SD-v1.5 tape in bf16, on the host): 159.7 GiB at max_batch 2 / 100 tangents, 79.9 GiB at 1 / 50, of the
# MI355X's 288 GB; --memory_bound lowers the group
TANGENT_BUDGET = 100


def tangent_space_group(args) -> int:
    """samples local_encoder_pullback_batch advances together in the tangent-space job: the pending pairs, bounded by memory_bound and TANGENT_BUDGET"""
    pairs = max(1, args.num_local_basis) * len(args.h_t_values)
    return max(1, min(pairs, args.memory_bound, TANGENT_BUDGET // max(args.pca_rank, 1)))


def transport_group(args) -> int:
    """samples whose local bases run_edit_parallel_transport computes together: the source and its targets, bounded like tangent_space_group"""
    samples = len(set([args.sample_idx_0] + list(args.sample_idx_1_values)))
    return max(1, min(samples, args.memory_bound, TANGENT_BUDGET // max(args.pca_rank, 1)))


def frechet_group(args) -> int:
    """local bases a global-basis job (run_edit_global_frechet_mean_zt, run_edit_global_flag_mean_zt, run_edit_global_hungarian_mean_zt) may have to sample together: up to num_local_basis, bounded like tangent_space_group"""
    return max(1, min(max(1, args.num_local_basis), args.memory_bound, TANGENT_BUDGET // max(args.pca_rank, 1)))


def build_unet(args) -> PullbackUNet:
    from . import weights as W
    small = args.net_scale != "full"
    # U-Net batch: memory_bound latents of the decode loop (x2 under classifier-free guidance), never below the 2 of x-space guidance
    max_batch = max(2, min(args.memory_bound, args.vis_num + 1) * (2 if args.guidance_scale > 1.0 else 1))
    if getattr(args, "trajectory_batch", 0) > 1 and args.is_stable_diffusion and args.run_edit_local_encoder_pullback_zt:
        # 2 * vis_num_pc chains together: batch 4 * vis_num_pc for the guidance step, 2 * vis_num_pc * (vis_num + 1) decode trajectories
        max_batch = max(max_batch, min(args.trajectory_batch, 2 * args.vis_num_pc * (args.vis_num + 1)) * (2 if args.guidance_scale > 1.0 else 1),
                        min(args.trajectory_batch, 4 * args.vis_num_pc))
    max_rank = max(args.pca_rank, 2)
    if getattr(args, "run_sample_encoder_local_tangent_space_zt", False):       # the group of (latent, h_t) pairs: batch and tangents for all of it
        max_batch = max(max_batch, tangent_space_group(args))
        max_rank = max(max_rank, tangent_space_group(args) * args.pca_rank)
    if getattr(args, "run_edit_parallel_transport", False):
        # the basis group: (1 + targets) samples x pca_rank tangents, in groups when that exceeds the budget ...
        max_batch = max(max_batch, transport_group(args))
        max_rank = max(max_rank, transport_group(args) * args.pca_rank)
        if getattr(args, "trajectory_batch", 0) > 1:
            # ... and the chains together: 2 * vis_num_pc per target and for the source, 2 rows each per guidance step, vis_num + 1 decode states each
            n = 2 * args.vis_num_pc * (1 + len(args.sample_idx_1_values))
            max_batch = max(max_batch, min(args.trajectory_batch, 2 * n), min(args.trajectory_batch, n * (args.vis_num + 1)))
    if (getattr(args, "run_edit_global_frechet_mean_zt", False) or getattr(args, "run_edit_global_hungarian_mean_zt", False)
            or getattr(args, "run_edit_global_flag_mean_zt", False)):
        # the local bases a global-basis job may have to sample, in groups; and the 2 * vis_num_pc chains together
        max_batch = max(max_batch, frechet_group(args))
        max_rank = max(max_rank, frechet_group(args) * args.pca_rank)
        if getattr(args, "trajectory_batch", 0) > 1:
            n = 2 * args.vis_num_pc
            max_batch = max(max_batch, min(args.trajectory_batch, 2 * n), min(args.trajectory_batch, n * (args.vis_num + 1)))
            if getattr(args, "edit_xt", "parallel-x") in ("parallel-h", "newton-h"):      # the chains of one inv_jac_chain call: a cotangent each (max_batch holds them already)
                max_rank = max(max_rank, min(args.trajectory_batch, n))
            if getattr(args, "edit_ht", "default") == "h_space_guidance":   # vis_num chains per experiment, a plain and a shifted row each per call
                max_batch = max(max_batch, min(args.trajectory_batch, 2 * n * args.vis_num))
    if getattr(args, "run_geodesic_interpolation", False):                     # the curve is one batch: its two ends and a cotangent per interior point
        max_batch = max(max_batch, args.geodesic_points + 2)
        max_rank = max(max_rank, args.geodesic_points)
    if args.is_stable_diffusion:
        cfg = cf.sd_config_for(args.model_name)           # SD-v1.x or SD-2(.1)-base; anything else raises
        if small:
            cfg = cf.SDConfig(block_out_channels=(32, 64), layers_per_block=1, down_attn=(True, False), up_attn=(False, True),
                              heads=(2, 2), cross_dim=64, groups=8, sample_size=16, use_linear_projection=cfg.use_linear_projection)
        params = torch.load(args.weights, map_location="cpu") if args.weights else cf.sd_init_params(cfg, seed=args.seed)
        W.check_shapes(params, cf.sd_param_shapes(cfg), f"{args.model_name} U-Net")
        if small:
            args.image_size = cfg.sample_size
        return PullbackUNet("sd", cfg, params, dtype=args.compute_dtype, device=args.device, max_batch=max_batch, max_rank=max_rank)
    if args.model_name in cf.ADM_MODEL_NAMES:             # the guided-diffusion U-Net (utils.py:68-99: g_DDPM + load_state_dict, names unchanged)
        cfg = cf.ADM_MODEL_NAMES[args.model_name]
        if small:
            cfg = cf.ADMConfig(image_size=32, model_channels=32, channel_mult=(1, 2, 2), num_res_blocks=1, attention_resolutions=(16,),
                               num_head_channels=16, use_scale_shift_norm=cfg.use_scale_shift_norm, resblock_updown=cfg.resblock_updown,
                               use_new_attention_order=cfg.use_new_attention_order, learn_sigma=cfg.learn_sigma)
        params = torch.load(args.weights, map_location="cpu") if args.weights else cf.adm_init_params(cfg, seed=args.seed)
        W.check_shapes(params, cf.adm_param_shapes(cfg), f"{args.model_name} U-Net")
        if small:
            args.image_size = cfg.image_size
        # eps is the first half of the output convolution (UNetModel.forward returns et): the scheduler keeps learn_sigma = False, as the reference's does
        return PullbackUNet("adm", cfg, params, dtype=args.compute_dtype, device=args.device, max_batch=max_batch, max_rank=max_rank)
    cfg = cf.CELEBA_HQ_256 if not small else cf.DDPMConfig(ch=32, ch_mult=(1, 2, 2), num_res_blocks=1, attn_resolutions=(16,), resolution=32)
    if args.weights:                                      # diffusers UNet2DModel keys (google/ddpm-ema-celebahq-256) or vendored names
        params = W.ddpm_hf_to_vendored_names(torch.load(args.weights, map_location="cpu"), cfg)
    else:
        params = cf.ddpm_init_params(cfg, seed=args.seed)
    W.check_shapes(params, cf.ddpm_param_shapes(cfg), f"{args.model_name} U-Net")
    if small:
        args.image_size = cfg.resolution
    return PullbackUNet("ddpm", cfg, params, dtype=args.compute_dtype, device=args.device, max_batch=max_batch, max_rank=max_rank)


def build_vae(args):
    """``pipe.vae`` of the reference (edit.py:144-146, :476-480) on the HIP engine; None keeps latents as the output."""
    if args.vae == "none" or not args.is_stable_diffusion:
        return None
    from .vae import AutoencoderKL
    small = args.net_scale != "full"
    cfg = cf.SD15_VAE if not small else cf.VAEConfig(block_out_channels=(32, 64), layers_per_block=1, groups=8, sample_size=2 * args.image_size)
    params = cf.vae_init_params(cfg, seed=args.seed) if args.vae == "synthetic" else torch.load(args.vae, map_location="cpu")
    return AutoencoderKL(cfg, params, dtype=args.compute_dtype, device=args.device, max_batch=1)


def build_prompt_encoder(args):
    """``pipe._encode_prompt`` of the reference (edit.py:505-522) on the HIP engine; None keeps the seeded stand-in
    embeddings.  The BPE tokenizer needs CLIP's vocabulary files (``--tokenizer_dir``, loaded with transformers'
    CLIPTokenizer); without them a byte-level stand-in tokenizer is used, which is only meaningful with synthetic weights."""
    if args.text_encoder == "none" or not args.is_stable_diffusion or args.net_scale != "full":
        return None
    from .text_encoder import ClipTextEncoder
    cfg = cf.clip_config_for(args.model_name)
    if args.tokenizer_dir:
        from transformers import CLIPTokenizer
        tk = CLIPTokenizer.from_pretrained(args.tokenizer_dir)
        tokenizer = lambda s: tk(s, padding="max_length", max_length=cfg.max_position, truncation=True).input_ids
    else:
        tokenizer = lambda s: ([cfg.vocab_size - 2] + [256 + b for b in s.encode()][: cfg.max_position - 2] + [cfg.vocab_size - 1] * cfg.max_position)[: cfg.max_position]
    params = cf.clip_init_params(cfg, seed=args.seed) if args.text_encoder == "synthetic" else torch.load(args.text_encoder, map_location="cpu")
    return ClipTextEncoder(cfg, params, dtype=args.compute_dtype, device=args.device, max_batch=1, tokenizer=tokenizer).encode_prompt


def main(argv=None):
    import time
    from . import timing as T
    t_start = time.perf_counter()
    args = preset(parse_args(argv))
    if getattr(args, "timing", False):
        T.enable(True)
    with T.phase("U-Net weights (synthetic draw / load) + engine build + upload"):
        unet = build_unet(args)
    if args.is_stable_diffusion:
        print("is stable-diffusion")
        with T.phase("VAE weights + engine build"):
            vae = build_vae(args)
        with T.phase("text-encoder weights + engine build"):
            penc = build_prompt_encoder(args)
        edit = EditStableDiffusion(args, unet=unet, vae=vae, prompt_encoder=penc)
    else:
        print("is NOT stable-diffusion")
        edit = EditUncondDiffusion(args, unet=unet)
    if args.run_edit_local_encoder_pullback_zt:                                  # main.py:30-34
        if args.is_stable_diffusion:
            edit.run_edit_local_encoder_pullback_zt(idx=args.sample_idx, op=args.op, block_idx=args.block_idx, vis_num=args.vis_num,
                                                    vis_num_pc=args.vis_num_pc, pca_rank=args.pca_rank, edit_prompt=args.edit_prompt)
        else:
            edit.run_edit_local_encoder_pullback_zt(idx=args.sample_idx, op=args.op, block_idx=args.block_idx, vis_num=args.vis_num,
                                                    vis_num_pc=args.vis_num_pc, pca_rank=args.pca_rank)
    if args.run_sample_encoder_local_tangent_space_zt:                           # main.py:45-91
        kw = dict(h_t=args.h_t_values if args.h_t_list else args.h_t, op=args.op, block_idx=args.block_idx, pca_rank=args.pca_rank,
                  num_local_basis=args.num_local_basis)
        if args.is_stable_diffusion:
            edit.run_sample_encoder_local_tangent_space_zt(use_edit_prompt=None, edit_prompt=args.edit_prompt, **kw)
        else:
            edit.run_sample_encoder_local_tangent_space_zt(fix_xt=args.fix_xt, fix_t=args.fix_t, **kw)
    if args.run_tangent_space_distance:                                          # after the sampling job when both are asked for: it reads that job's files
        kw = dict(h_t=args.h_t_values if args.h_t_list else args.h_t, op=args.op, block_idx=args.block_idx, pca_rank=args.pca_rank,
                  num_local_basis=args.num_local_basis, space=args.distance_space)
        if args.is_stable_diffusion:
            edit.run_tangent_space_distance(edit_prompt=args.edit_prompt, **kw)
        else:
            edit.run_tangent_space_distance(fix_xt=args.fix_xt, fix_t=args.fix_t, **kw)
    if args.run_tangent_space_clusters:                                          # likewise after the sampling job
        kw = dict(h_t=args.h_t_values if args.h_t_list else args.h_t, op=args.op, block_idx=args.block_idx, pca_rank=args.pca_rank,
                  num_local_basis=args.num_local_basis, space=args.distance_space, num_clusters=args.num_clusters,
                  cluster_rank=args.cluster_rank or None)
        if args.is_stable_diffusion:
            edit.run_tangent_space_clusters(edit_prompt=args.edit_prompt, **kw)
        else:
            edit.run_tangent_space_clusters(fix_xt=args.fix_xt, fix_t=args.fix_t, **kw)
    if args.run_tangent_space_pga:                                               # likewise after the sampling job
        kw = dict(h_t=args.h_t_values if args.h_t_list else args.h_t, op=args.op, block_idx=args.block_idx, pca_rank=args.pca_rank,
                  num_local_basis=args.num_local_basis, space=args.distance_space, pga_base=args.pga_base, pga_modes=args.pga_modes or None)
        if args.is_stable_diffusion:
            edit.run_tangent_space_pga(edit_prompt=args.edit_prompt, **kw)
        else:
            edit.run_tangent_space_pga(fix_xt=args.fix_xt, fix_t=args.fix_t, **kw)
    if args.run_edit_parallel_transport:                                         # main.py:36-40 (which fixes op='mid', block_idx=0, vis_num=4, vis_num_pc=2, pca_rank=50)
        edit.run_edit_parallel_transport(sample_idx_0=args.sample_idx_0,
                                         sample_idx_1=args.sample_idx_1_values if args.sample_idx_1_list else args.sample_idx_1, op=args.op,
                                         block_idx=args.block_idx, vis_num=args.vis_num, vis_num_pc=args.vis_num_pc, pca_rank=args.pca_rank,
                                         h_t=args.h_t)
    if args.run_geodesic_interpolation:                                          # (not in the reference: the shortest path under its paper's metric)
        edit.run_geodesic_interpolation(sample_idx_0=args.sample_idx_0, sample_idx_1=args.sample_idx_1, op=args.op, block_idx=args.block_idx,
                                        h_t=args.h_t, n_points=args.geodesic_points, lam=args.geodesic_lambda, max_iter=args.geodesic_max_iter,
                                        tol=args.geodesic_tol)
    if args.run_edit_global_frechet_mean_zt:                                     # (the reference's main.py never calls it; its method's own defaults otherwise)
        edit.run_edit_global_frechet_mean_zt(idx=args.sample_idx, op=args.op, block_idx=args.block_idx, vis_num=args.vis_num, vis_num_pc=args.vis_num_pc,
                                             pca_rank=args.pca_rank, num_local_basis=args.num_local_basis, local_projection=args.local_projection,
                                             frechet_mean_space=args.frechet_mean_space, h_t=args.h_t, frechet_max_iter=args.frechet_max_iter,
                                             frechet_tol=args.frechet_tol, frechet_init=args.frechet_init)
    if args.run_edit_global_flag_mean_zt:                                        # (not in the reference: the third global basis)
        edit.run_edit_global_flag_mean_zt(idx=args.sample_idx, op=args.op, block_idx=args.block_idx, vis_num=args.vis_num, vis_num_pc=args.vis_num_pc,
                                          pca_rank=args.pca_rank, num_local_basis=args.num_local_basis, local_projection=args.local_projection,
                                          flag_mean_space=args.flag_mean_space, h_t=args.h_t, flag_rank=args.flag_rank,
                                          flag_mean_kind=args.flag_mean_kind, flag_median_eps=args.flag_median_eps,
                                          flag_median_max_rounds=args.flag_median_max_rounds)
    if args.run_edit_global_hungarian_mean_zt:                                   # (the reference's main.py never calls it; its method's own defaults otherwise)
        edit.run_edit_global_hungarian_mean_zt(idx=args.sample_idx, op=args.op, block_idx=args.block_idx, vis_num=args.vis_num,
                                               vis_num_pc=args.vis_num_pc, pca_rank=args.pca_rank, num_local_basis=args.num_local_basis,
                                               local_projection=args.local_projection, hungarian_mean_space=args.hungarian_mean_space, h_t=args.h_t,
                                               hungarian_distance=args.hungarian_distance, hungarian_max_sweeps=args.hungarian_max_sweeps)
    if args.run_ddim_forward:
        edit.run_DDIMforward(num_samples=5)
    if args.run_ddim_inversion:
        edit.run_DDIMinversion(idx=args.sample_idx)
    if T.ENABLED:
        print(T.report(time.perf_counter() - t_start))
    return edit


if __name__ == "__main__":
    main(sys.argv[1:])
