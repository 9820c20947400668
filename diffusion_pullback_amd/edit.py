"""Experiment drivers of the pullback editing path, latents resident on the device.

Mirrors the public surface of the reference's ``modules/edit.py``:
  * ``EditStableDiffusion``  (reference src/modules/edit.py:31-535)
      run_DDIMinversion :112-183, run_edit_local_encoder_pullback_zt :185-307, run_sample_encoder_local_tangent_space_zt :310-383,
      DDIMforwardsteps :385-482, x_space_guidance :484-502, run_DDIMforward :101-110
  * ``EditUncondDiffusion``  (reference src/modules/edit.py:540-779, :1601-1734)
      run_DDIMinversion :613-678, run_edit_local_encoder_pullback_zt :680-779, run_edit_parallel_transport :782-948,
      run_edit_global_frechet_mean_zt :951-1246 (its global basis: geometry.frechet_mean),
      run_edit_global_hungarian_mean_zt :1249-1514 (its global bases: geometry.hungarian_mean),
      run_edit_global_flag_mean_zt (not in the reference; a third global basis: geometry.flag_mean),
      run_sample_encoder_local_tangent_space_zt :1517-1599, DDIMforwardsteps :1601-1714, x_space_guidance :1716-1734

Kept from the reference: the step counts (inv_steps-2 inversion steps, ``edit_t_idx`` forward steps,
``x_space_guidance_num_step`` guidance steps, the rest decode), the ``[::len // vis_num]`` subsample,
the u / vT normalisation, the ``.pt`` basis cache naming, EXP_NAME / result file naming, the
"already done" skips and the eta=1 "performance boosting" tail of the unconditional decode.
Changed on purpose: latents never bounce through a CPU buffer (the reference moves them every
step, edit.py:434, :469-472); chunks of ``memory_bound`` samples still bound the U-Net batch.

Third-party pieces the reference takes from diffusers (VAE, CLIP prompt encoder, image datasets) are
injected: ``vae`` (``encode(x)->latent``, ``decode(z)->image``), ``prompt_encoder(str)->[1,L,D]``,
``dataset[idx]->[1,3,H,W]``.  Without them the drivers run on synthetic latents / seeded prompt
embeddings and save latents instead of decoded images (there are no weights offline).
"""
from __future__ import annotations

import math
import os
import zlib
from typing import Optional

import torch

from . import timing as T
from .scheduler import get_custom_diffusion_scheduler, get_stable_diffusion_scheduler


def save_image(x: torch.Tensor, path: str, nrow: Optional[int] = None) -> None:
    """Minimal stand-in for torchvision.utils.save_image (edit.py:480): images in [0,1], one row."""
    x = x.detach().float().clamp(0, 1).cpu()
    if x.dim() == 2:                                   # a matrix (the unconditional driver saves the raw vT): one grey image
        x = x[None, None]
    if x.dim() == 3:
        x = x[None]
    if x.shape[1] not in (1, 3):                       # latents: keep as tensor next to the requested name
        torch.save(x, os.path.splitext(path)[0] + ".pt")
        return
    try:
        from PIL import Image
        row = torch.cat(list(x), dim=2)                # [C, H, B*W]
        arr = (row.permute(1, 2, 0) * 255 + 0.5).to(torch.uint8).numpy()
        Image.fromarray(arr.squeeze(-1) if arr.shape[-1] == 1 else arr).save(path, compress_level=1)   # same pixels, a third of the default level's encode time
    except Exception:
        torch.save(x, os.path.splitext(path)[0] + ".pt")


def save_spectrum_plot(s: torch.Tensor, path: str, dpi=None) -> None:
    """Scatter plot of the singular values next to the cached basis (edit.py:249-251 / :733-735); skipped without matplotlib."""
    try:
        import matplotlib
        matplotlib.use("Agg", force=False)
        import matplotlib.pyplot as plt
    except Exception:
        return
    plt.scatter(range(s.size(0)), s.detach().float().cpu().tolist(), s=1)
    plt.savefig(path, **({"dpi": dpi} if dpi else {}))
    plt.close()


def save_distance_plot(dist: torch.Tensor, path: str, dpi=None) -> None:
    """Heat map of a matrix of geodesic distances next to its .pt file (the matplotlib route of save_spectrum_plot); skipped without matplotlib."""
    try:
        import matplotlib
        matplotlib.use("Agg", force=False)
        import matplotlib.pyplot as plt
    except Exception:
        return
    plt.imshow(dist.detach().float().cpu().numpy(), cmap="viridis")
    plt.colorbar(label="geodesic distance (rad)")
    plt.savefig(path, **({"dpi": dpi} if dpi else {}))
    plt.close()


def save_pga_plots(variance, scores: torch.Tensor, h_t, scree_path: str, scatter_path: str, dpi=None) -> None:
    """The scree plot of a tangent-space PGA (variance per mode) and the scatter of its first two score columns coloured by h_t, next to its .pt file
    (one column: the scores against the member index); skipped without matplotlib."""
    try:
        import matplotlib
        matplotlib.use("Agg", force=False)
        import matplotlib.pyplot as plt
    except Exception:
        return
    kw = {"dpi": dpi} if dpi else {}
    v = torch.as_tensor(variance).double().numpy()
    plt.plot(range(1, len(v) + 1), v, "o-")
    plt.xlabel("mode")
    plt.ylabel("variance (rad^2)")
    plt.savefig(scree_path, **kw)
    plt.close()
    s = scores.detach().double().cpu().numpy()
    x, y = (s[:, 0], s[:, 1]) if s.shape[1] > 1 else (range(len(s)), s[:, 0])
    plt.scatter(x, y, c=[float(h) for h in h_t], cmap="viridis")
    plt.colorbar(label="h_t")
    plt.xlabel("score 1" if s.shape[1] > 1 else "member")
    plt.ylabel("score 2" if s.shape[1] > 1 else "score 1")
    plt.savefig(scatter_path, **kw)
    plt.close()


def save_projection_plot(cu: Optional[torch.Tensor], cv: torch.Tensor, path: str) -> None:
    """The sorted magnitudes of a direction's coefficients in the local basis, 'u' (h-space; None: there is no h-space direction) and 'v' (x-space):
    projection_coeff-<EXP_NAME>.png of the global-basis job (edit.py:1168-1172); skipped without matplotlib."""
    try:
        import matplotlib
        matplotlib.use("Agg", force=False)
        import matplotlib.pyplot as plt
    except Exception:
        return
    for c, label in ((cu, "u"), (cv, "v")):
        if c is not None:
            plt.scatter(range(c.numel()), sorted(c.detach().float().abs().cpu().tolist()), label=label)
    plt.legend()
    plt.savefig(path, dpi=80)
    plt.close()


def save_vT_visualisation(vT: torch.Tensor, lat_shape, path: str) -> None:
    """vT [k, N_in] shown through the 3 principal channel directions of its pixels, min-max normalised (edit.py:253-263, :359-369)"""
    pix = vT.view(-1, *lat_shape).permute(0, 2, 3, 1).reshape(-1, lat_shape[0]).float()
    _, _, basis = torch.pca_lowrank(pix, q=min(3, pix.shape[1]), center=True, niter=2)
    vis = torch.einsum("bcwh,cp->bpwh", vT.view(-1, *lat_shape).float(), basis)
    vis = vis - vis.min()
    save_image(vis / vis.max(), path)


class _SeededPrompts:
    """Stand-in for pipe._encode_prompt (edit.py:505-522): a deterministic embedding per prompt string."""

    def __init__(self, length: int, dim: int):
        self.length, self.dim = length, dim

    def __call__(self, prompt: str) -> torch.Tensor:
        g = torch.Generator().manual_seed(zlib.crc32(prompt.encode()) if prompt else 0)
        return torch.randn(1, self.length, self.dim, generator=g)


class _EditBase(object):
    latent_scale = 1.0

    def _chunks(self, x, per_sample: int = 1):
        """Batches of at most ``memory_bound`` samples (edit.py:434-438), further bounded by the engine's own batch limit
        (``per_sample`` = 2 under classifier-free guidance, which doubles the U-Net batch).  Samples are independent, so the
        batching is not observable in the result."""
        cap = getattr(getattr(self.unet, "engine", None), "max_batch", None)
        want = max(self.memory_bound, getattr(self, "trajectory_batch", 0))      # trajectory batching (below) raises the bound on purpose
        bound = want if cap is None else max(1, min(want, cap // per_sample))
        return list(x.split(bound))

    _phase = "U-Net forward (other)"

    def _eps(self, x, t, emb=None):
        with T.phase(self._phase):
            out = self.unet(x, t) if emb is None else self.unet(x, t, encoder_hidden_states=emb)
        return out if isinstance(out, torch.Tensor) else out.sample

    def _basis_paths(self, save_dir, name):
        os.makedirs(save_dir, exist_ok=True)
        return [os.path.join(save_dir, p + name + ".pt") for p in ("u-", "s-", "vT-")]

    def _random_latent(self, idx):
        """dataset 'Random': entry idx of a dataset of Gaussian latents (the caller's dataset, or one seeded by (seed, idx): the same latent
        whenever idx is asked for, as a dataset entry is)"""
        if self.dataset is not None:
            return self.dataset[idx].to(device=self.device, dtype=self.dtype)
        return self._seeded_latent(idx)

    def _seeded_latent(self, idx):
        g = torch.Generator().manual_seed((int(self.seed) << 20) + int(idx))
        return torch.randn(1, self.c_in, self.image_size, self.image_size, generator=g).to(device=self.device, dtype=self.dtype)

    def _pending_tangent_spaces(self, h_t, num_local_basis, save_dir, exp_name):
        """the (basis index, h_t) pairs still to sample, in the reference's order (h_t outer, basis index inner), with their EXP_NAME and files;
        a pair whose u-, s- and vT- files all exist is skipped (edit.py:337-339, :1560-1562)"""
        os.makedirs(save_dir, exist_ok=True)
        pending = []
        for idx, ht, name, paths in self._tangent_space_pairs(h_t, num_local_basis, save_dir, exp_name):
            if all(os.path.exists(p) for p in paths):
                print(f"!!!ALREADY SAMPLED LOCAL BASIS IDX : {idx}!!!")
                continue
            pending.append((idx, ht, name, paths))
        return pending

    def _tangent_space_pairs(self, h_t, num_local_basis, save_dir, exp_name):
        """every (basis index, h_t) pair of the job in the reference's order (h_t outer, basis index inner), with its EXP_NAME and its u- / s- / vT- files"""
        return [(idx, ht, exp_name(idx, ht), [os.path.join(save_dir, p + exp_name(idx, ht) + ".pt") for p in ("u-", "s-", "vT-")])
                for ht in (list(h_t) if isinstance(h_t, (list, tuple)) else [h_t]) for idx in range(num_local_basis)]

    @torch.no_grad()
    def run_tangent_space_distance(self, h_t, op, block_idx, pca_rank=50, num_local_basis=10, space="x", max_bytes=None, **naming):
        """Principal angles and geodesic distances between the local tangent spaces run_sample_encoder_local_tangent_space_zt saved -- the
        analysis those files are for (the reference has no code for it).  The job's (basis index, h_t) pairs are listed in the order of
        _pending_tangent_spaces, in the directory and under the EXP_NAMEs of the sampling job (naming: what the driver's
        _tangent_space_naming takes -- edit_prompt for Stable Diffusion, fix_xt / fix_t for the unconditional nets).  space "x": the row spans of
        vT [k, N_in]; "h": the column spans of u [N_h, k] (un-normalised J V: the angles do not need orthonormal rows).  Nothing is sampled here:
        a missing file raises ValueError with the list of missing names.  The stack goes to the device and through geometry.py (dpb_subspace_angles,
        self mode).  Writes tangent_space_distance-<space>-<EXP_NAME of the set>.pt -- a dict of names, idx, h_t, theta [P, P, k] (descending) and
        dist [P, P] = ||theta||_2 -- and a heat map of dist as .png next to it; returns the dict.  Distances only: no means, no transport."""
        from . import geometry
        if space not in ("x", "h"):
            raise ValueError(f"space must be 'x' (vT) or 'h' (u), got {space!r}")
        save_dir, exp_name = self._tangent_space_naming(op, block_idx, pca_rank, **naming)
        pairs = self._tangent_space_pairs(h_t, num_local_basis, save_dir, exp_name)
        files = [paths[2] if space == "x" else paths[0] for _, _, _, paths in pairs]
        missing = [os.path.basename(f) for f in files if not os.path.exists(f)]
        if missing:
            raise ValueError(f"{len(missing)} of {len(files)} tangent-space files are missing in {save_dir}: {missing}; run the sampling job "
                             "(run_sample_encoder_local_tangent_space_zt) with the same arguments first")
        with T.phase("tangent-space distances (principal angles)"):
            bases = [torch.load(f, map_location=self.device).float() for f in files]
            stack = torch.stack([b if space == "x" else b.T for b in bases]).contiguous()
            theta, dist = geometry.subspace_angles_and_distance(stack, None, max_bytes)
        hts = list(h_t) if isinstance(h_t, (list, tuple)) else [h_t]
        self.EXP_NAME = f"tangent_space_distance-{space}-" + exp_name(f"0to{num_local_basis - 1}", ",".join(str(h) for h in hts))
        out = dict(names=[name for _, _, name, _ in pairs], idx=[int(i) for i, _, _, _ in pairs], h_t=[float(h) for _, h, _, _ in pairs],
                   theta=theta.cpu(), dist=dist.cpu())
        torch.save(out, os.path.join(save_dir, self.EXP_NAME + ".pt"))
        save_distance_plot(out["dist"], os.path.join(save_dir, self.EXP_NAME + ".png"), dpi=80)
        return out

    @torch.no_grad()
    def run_tangent_space_clusters(self, h_t, op, block_idx, pca_rank=50, num_local_basis=10, space="x", num_clusters=2, cluster_rank=None,
                                   max_bytes=None, **naming):
        """Flag k-means of the local tangent spaces run_sample_encoder_local_tangent_space_zt saved: the (basis index, h_t) pairs clustered into
        num_clusters families, each with a rank-cluster_rank (None: pca_rank) flag mean as its centre (geometry.flag_kmeans) -- where every other
        consumer of many bases assumes one global basis for the whole set.  The files are listed, named and refused as run_tangent_space_distance
        does (a missing one raises ValueError naming it; nothing is sampled); space "x": the row spans of vT, "h": the column spans of u.  Writes
        tangent_space_clusters-<space>-C<C>-r<r>-<EXP_NAME of the set>.pt -- a dict of names, idx, h_t, labels [P], centres [C, r, N], affinity
        [P, C], objective, weight [C, r], gap, sizes, converged -- and a heat map of r - affinity, rows sorted by label, as .png next to it; prints
        every cluster's size and its spectrum around row r, so that a missing gap is seen.  Returns the dict."""
        from . import geometry
        if space not in ("x", "h"):
            raise ValueError(f"space must be 'x' (vT) or 'h' (u), got {space!r}")
        save_dir, exp_name = self._tangent_space_naming(op, block_idx, pca_rank, **naming)
        pairs = self._tangent_space_pairs(h_t, num_local_basis, save_dir, exp_name)
        files = [paths[2] if space == "x" else paths[0] for _, _, _, paths in pairs]
        missing = [os.path.basename(f) for f in files if not os.path.exists(f)]
        if missing:
            raise ValueError(f"{len(missing)} of {len(files)} tangent-space files are missing in {save_dir}: {missing}; run the sampling job "
                             "(run_sample_encoder_local_tangent_space_zt) with the same arguments first")
        r = int(cluster_rank) if cluster_rank else int(pca_rank)
        with T.phase("tangent-space clusters (flag k-means)"):
            bases = [torch.load(f, map_location=self.device).float() for f in files]
            stack = torch.stack([b if space == "x" else b.T for b in bases]).contiguous()
            labels, centres, info = geometry.flag_kmeans(stack, int(num_clusters), rank=r, max_bytes=max_bytes)
        hts = list(h_t) if isinstance(h_t, (list, tuple)) else [h_t]
        self.EXP_NAME = f"tangent_space_clusters-{space}-C{int(num_clusters)}-r{r}-" + exp_name(f"0to{num_local_basis - 1}", ",".join(str(h) for h in hts))
        out = dict(names=[name for _, _, name, _ in pairs], idx=[int(i) for i, _, _, _ in pairs], h_t=[float(h) for _, h, _, _ in pairs],
                   labels=labels.cpu(), centres=centres.cpu(), affinity=info["affinity"].cpu(), objective=torch.as_tensor(info["objective"]),
                   weight=info["weight"].cpu(), gap=info["gap"], sizes=torch.as_tensor(info["sizes"]), converged=info["converged"])
        for c, eig in enumerate(info["eigenvalues"]):
            lo, hi = max(0, r - 3), min(len(eig), r + 3)
            around = " ".join(f"{v:.3f}" for v in eig[lo:r]) + " | " + " ".join(f"{v:.3f}" for v in eig[r:hi])
            print(f"cluster {c}: {int(info['sizes'][c])} members, spectrum rows {lo}..{hi - 1} (| after row {r}): {around}, gap {info['gap'][c]}")
        torch.save(out, os.path.join(save_dir, self.EXP_NAME + ".pt"))
        order = torch.argsort(out["labels"], stable=True)
        save_distance_plot((r - out["affinity"])[order], os.path.join(save_dir, self.EXP_NAME + ".png"), dpi=80)
        return out

    @torch.no_grad()
    def run_tangent_space_pga(self, h_t, op, block_idx, pca_rank=50, num_local_basis=10, space="x", pga_base="frechet", pga_modes=None, max_bytes=None,
                              **naming):
        """Principal geodesic analysis of the local tangent spaces run_sample_encoder_local_tangent_space_zt saved: how the (basis index, h_t) pairs
        vary around a centre -- the modes that carry the spread, where every pair sits on them and, when the files span more than one h_t, how much
        of the spread is a trend in the timestep (geometry.grassmann_pga with the h_t of each file as the covariate).  The files are listed, named and
        refused as run_tangent_space_distance does (a missing one raises ValueError naming it; nothing is sampled); space "x": the row spans of vT,
        "h": the column spans of u.  pga_base: "frechet" (the Karcher mean), "flag" (the flag mean) or a member's position in the list; pga_modes:
        None for grassmann_pga's default.  Writes tangent_space_pga-<space>-<base>-M<M>-<EXP_NAME of the set>.pt -- a dict of names, idx, h_t, base
        [k, N], modes [M, k, N], variance, explained, scores [P, M], residual, theta, mean_tangent_norm and, when fitted, slopes, intercept, r2,
        slope_norm -- with a scree plot (-scree.png) and a scatter of the first two score columns coloured by h_t (-scores.png) next to it; prints
        the spectrum and r2.  A mode is a tangent at the base: geometry.grassmann_exp(base, t * modes[m], 1.0) is a basis to edit with.  Returns
        the dict."""
        from . import geometry
        if space not in ("x", "h"):
            raise ValueError(f"space must be 'x' (vT) or 'h' (u), got {space!r}")
        if not (pga_base in ("frechet", "flag") or (isinstance(pga_base, int) and not isinstance(pga_base, bool))):
            raise ValueError(f"pga_base must be 'frechet', 'flag' or the position of a member, got {pga_base!r}")
        save_dir, exp_name = self._tangent_space_naming(op, block_idx, pca_rank, **naming)
        pairs = self._tangent_space_pairs(h_t, num_local_basis, save_dir, exp_name)
        files = [paths[2] if space == "x" else paths[0] for _, _, _, paths in pairs]
        missing = [os.path.basename(f) for f in files if not os.path.exists(f)]
        if missing:
            raise ValueError(f"{len(missing)} of {len(files)} tangent-space files are missing in {save_dir}: {missing}; run the sampling job "
                             "(run_sample_encoder_local_tangent_space_zt) with the same arguments first")
        hts = list(h_t) if isinstance(h_t, (list, tuple)) else [h_t]
        member_ht = [float(h) for _, h, _, _ in pairs]
        trend = len(set(member_ht)) > 1
        with T.phase("tangent-space PGA (principal geodesic analysis)"):
            bases = [torch.load(f, map_location=self.device).float() for f in files]
            stack = torch.stack([b if space == "x" else b.T for b in bases]).contiguous()
            base, modes, info = geometry.grassmann_pga(stack, base=pga_base, n_modes=None if not pga_modes else int(pga_modes),
                                                       covariates=member_ht if trend else None, max_bytes=max_bytes)
        m = modes.shape[0]
        self.EXP_NAME = f"tangent_space_pga-{space}-{pga_base}-M{m}-" + exp_name(f"0to{num_local_basis - 1}", ",".join(str(h) for h in hts))
        out = dict(names=[name for _, _, name, _ in pairs], idx=[int(i) for i, _, _, _ in pairs], h_t=member_ht, base=base.cpu(), modes=modes.cpu(),
                   variance=torch.as_tensor(info["variance"]), explained=torch.as_tensor(info["explained"]), scores=info["scores"].cpu(),
                   residual=info["residual"].cpu(), theta=info["theta"].cpu(), mean_tangent_norm=info["mean_tangent_norm"])
        if trend:
            out.update(slopes=info["slopes"].cpu(), intercept=info["intercept"].cpu(), r2=info["r2"], slope_norm=torch.as_tensor(info["slope_norm"]))
        print(f"tangent-space PGA at the {pga_base} base, {len(pairs)} members: variance " + " ".join(f"{v:.3e}" for v in info["variance"])
              + f"; explained {info['explained'][-1]:.3f} of {info['total_variance']:.3e}" + (f"; trend in h_t: r2 {info['r2']:.3f}" if trend else ""))
        path = os.path.join(save_dir, self.EXP_NAME)
        torch.save(out, path + ".pt")
        save_pga_plots(out["variance"], out["scores"], member_ht, path + "-scree.png", path + "-scores.png", dpi=80)
        return out

    @torch.no_grad()
    def run_geodesic_interpolation(self, sample_idx_0, sample_idx_1, op, block_idx, h_t=None, n_points=8, lam=0.0, max_iter=200, tol=1e-4,
                                   check_every=4, max_halvings=8):
        """The shortest path between two samples under the pullback metric of h = get_h(x, t) at the tap (op, block_idx), beside the two
        interpolations a user has otherwise (the reference has no such job; its paper's metric is this one).  Both samples go to h_t (None: edit_t)
        the way the tangent-space job takes its latents there: inversion or a Random latent, then DDIMforwardsteps.  The geodesic of n_points interior
        points starts from the slerp curve (unet.pullback_geodesic: lam, max_iter, tol, check_every, max_halvings); lerp, slerp and geodesic are then
        measured alike by unet.curve_energy and decoded together from h_t through DDIMforwardsteps(.., t_end_idx=-1) under the driver's batch bounds.
        Files: x0_gen-Geodesic-<dataset>_<i>_<j>-<h_t>T-<op>-block_<b>-{lerp|slerp|geodesic}.png in the result folder, one row per curve, and
        geodesic-Geodesic-<...>.pt in the obs folder: names, seed, h_t, t, the three curves at h_t, their statistics (energy, energy_h, energy_x,
        length_h, length_x, uniformity, seg_h, seg_x) and the info of pullback_geodesic.  An existing .pt is loaded, not recomputed.  Prints one
        line per curve; returns the record."""
        from .pullback import geodesic_init
        if int(sample_idx_0) == int(sample_idx_1):
            raise ValueError(f"run_geodesic_interpolation joins two different samples, got sample_idx_0 = sample_idx_1 = {sample_idx_0}")
        if int(n_points) < 1 or not (0 <= float(lam) < float("inf")):
            raise ValueError(f"run_geodesic_interpolation: n_points={n_points} must be >= 1 and lam={lam} finite and >= 0")
        h_t = self.edit_t if h_t is None else h_t
        name = f"Geodesic-{self.dataset_name}_{sample_idx_0}_{sample_idx_1}-{h_t}T-{op}-block_{block_idx}"
        self.EXP_NAME = name
        kinds = ("lerp", "slerp", "geodesic")
        line = lambda k, s: print(f"{name} {k}: energy {s['energy']:.6e}  h-length {s['length_h']:.6e}  uniformity {s['uniformity']:.6f}")
        path = os.path.join(self.obs_folder, f"geodesic-{name}.pt")
        if os.path.exists(path):
            print("!!!ALREADY DONE!!!")
            rec = torch.load(path)
            for k in kinds:
                line(k, rec["stats"][k])
            return rec
        self.scheduler.set_timesteps(self.for_steps, device=self.device)
        h_t_idx = int((self.scheduler.timesteps - h_t * 1000).abs().argmin())
        ends, t = [], self.scheduler.timesteps[h_t_idx]
        for idx in (sample_idx_0, sample_idx_1):
            xT = self._random_latent(idx) if self.dataset_name == "Random" else self.run_DDIMinversion(idx=idx)
            ends.append(xT if h_t_idx == 0 else self.DDIMforwardsteps(xT, t_start_idx=0, t_end_idx=h_t_idx)[0])
        xa, xb = (e.to(device=self.device, dtype=self.dtype) for e in ends)
        ctx = self._geodesic_ctx()
        with T.phase("pullback geodesic (device energy chain)"):
            geo, info = self.unet.pullback_geodesic(xa, xb, t, n_points=int(n_points), op=op, block_idx=block_idx, encoder_hidden_states=ctx,
                                                    init="slerp", lam=float(lam), max_iter=int(max_iter), tol=float(tol), check_every=int(check_every),
                                                    max_halvings=int(max_halvings))
            curves = {"lerp": geodesic_init(xa[0], xb[0], int(n_points), "linear"), "slerp": geodesic_init(xa[0], xb[0], int(n_points), "slerp"),
                      "geodesic": geo.to(device=self.device, dtype=torch.float32)}
            stats = {k: self.unet.curve_energy(curves[k], t, op=op, block_idx=block_idx, encoder_hidden_states=ctx, lam=float(lam)) for k in kinds}
        for k in kinds:
            line(k, stats[k])
        self._geodesic_decode(torch.cat([curves[k] for k in kinds]).to(self.dtype), h_t_idx, [f"{name}-{k}" for k in kinds])
        self.EXP_NAME = name
        rec = dict(names=[f"{name}-{k}" for k in kinds], seed=self.seed, h_t=float(h_t), t=float(t), op=op, block_idx=block_idx, n_points=int(n_points),
                   lam=float(lam), sample_idx=(int(sample_idx_0), int(sample_idx_1)), curves={k: curves[k].cpu() for k in kinds}, stats=stats, info=info)
        torch.save(rec, path)
        return rec

    def _guidance_chains_together(self, z, vk, t, emb=None):
        """n independent chains of x-space guidance (edit.py:484-502, :1716-1734) advanced together: chain i starts at z[i] and moves along vk[i],
        all at the timestep t.  Per step ONE U-Net call of 2 n rows, [z_1..z_n | z_1 + s v_1 .. z_n + s v_n], split only by the engine's batch limit
        and an explicit --memory_bound (the pair of a chain is never split).  emb: the [1, L, D] conditioning of every row (None: an unconditional
        net).  Returns the states [n, x_space_guidance_num_step + 1, ...], the start included."""
        n = z.size(0)
        chain = [z]
        cap = getattr(getattr(self.unet, "engine", None), "max_batch", None) or 2 * n
        per = max(1, min(n, cap // 2))                                                          # chains per U-Net call
        if getattr(self, "memory_bound_given", None):
            per = max(1, min(per, self.memory_bound_given // 2))
        for _ in range(self.x_space_guidance_num_step):
            nxt = []
            for zc, vc in zip(z.split(per), vk.split(per)):
                m = zc.size(0)
                et = self._eps(torch.cat([zc, zc + self.x_space_guidance_edit_step * vc], dim=0), t,
                               None if emb is None else emb.repeat(2 * m, 1, 1))                # edit.py:490
                et_null, et_edit = et.chunk(2)
                nxt.append(zc + self.x_space_guidance_scale * (et_edit - et_null))              # edit.py:501
            z = torch.cat(nxt, dim=0)
            chain.append(z)
        return torch.stack(chain, dim=1)

    def _sample_tangent_spaces(self, pending, make_xt, ctx, op, block_idx, pca_rank, thr, save_dir, finish):
        """The pending pairs through unet.local_encoder_pullback_batch, in groups of at most min(max_batch, max_rank // pca_rank): the samples of
        a group -- each at its own (x_t, t) -- advance together, each stopped by its own rule.  make_xt(idx, h_t) -> (x_t [1, ...], t) is
        called group by group; finish(name, s, vT, lat_shape) writes the pictures of one basis.  min_iter / max_iter: the reference's call-site
        constants (edit.py:354-357, :1581-1584)."""
        eng = getattr(self.unet, "engine", None)
        group = min(getattr(eng, "max_batch", 1), getattr(self.unet, "max_rank", pca_rank) // pca_rank)
        if group < 1:
            raise ValueError(f"pca_rank={pca_rank} exceeds the {getattr(self.unet, 'max_rank', None)} tangents this U-Net engine was built for")
        self.last_tangent_inputs = {}                          # (basis index, h_t) -> (x_t, t) of this call (introspection for tests)
        for g0 in range(0, len(pending), group):
            part = pending[g0:g0 + group]
            xs, ts = [], []
            for idx, ht, name, _ in part:
                print(f"!!!SAMPLE LOCAL BASIS IDX : {idx}!!!")
                xt, t = make_xt(idx, ht)
                xs.append(xt.to(device=self.device, dtype=self.dtype)); ts.append(float(t))
                self.last_tangent_inputs[(idx, ht)] = (xs[-1], ts[-1])
            with T.phase("local_encoder_pullback_batch (power iteration)"):
                u, s, vT, _ = self.unet.local_encoder_pullback_batch(torch.cat(xs, dim=0), torch.tensor(ts), ctx, op=op, block_idx=block_idx,
                                                                     pca_rank=pca_rank, min_iter=10, max_iter=50, convergence_threshold=thr)
            for b, (idx, ht, name, (u_path, s_path, vT_path)) in enumerate(part):
                ub, sb, vb = u[b].clone(), s[b].clone(), vT[b].clone()      # (clones: a saved view would carry the whole group's storage)
                finish(name, sb, vb, xs[b].shape[1:])
                save_spectrum_plot(sb, os.path.join(save_dir, f"eigenvalue_spectrum-{name}.png"), dpi=80)   # edit.py:374-377, :1586-1589
                torch.save(ub, u_path); torch.save(sb, s_path); torch.save(vb, vT_path)


# =================================================================== Stable Diffusion
class EditStableDiffusion(_EditBase):
    def __init__(self, args, unet=None, vae=None, prompt_encoder=None, dataset=None, scheduler=None):
        self.seed = args.seed
        self.memory_bound = getattr(args, "memory_bound", 5)
        # > 1: the 2 * vis_num_pc independent (pc, +-) edits of run_edit_local_encoder_pullback_zt advance TOGETHER -- their x-space-guidance chains
        # in one U-Net call per step, their decode trajectories in one batch -- instead of one after another as edit.py:276-307 does.  Samples are
        # independent in every kernel, so files, names and tensors are the same; the GPU sees 4x fewer, 4x fatter launches.  0 / 1: the reference's order.
        self.trajectory_batch = int(getattr(args, "trajectory_batch", 0) or 0)
        self.memory_bound_given = getattr(args, "memory_bound_given", None)      # explicit --memory_bound: bounds every U-Net call (floor: the pair of x-space guidance)
        self.unet = unet
        self.vae = vae
        self.dtype = getattr(args, "dtype", torch.float32)
        self.device = torch.device(args.device)
        self.scheduler = get_stable_diffusion_scheduler(args, scheduler)
        self.for_steps, self.inv_steps = args.for_steps, args.inv_steps
        self.use_yh_custom_scheduler = args.use_yh_custom_scheduler
        self.c_in, self.image_size = getattr(args, "c_in", 4), getattr(args, "image_size", 64)
        self.dataset = dataset
        self.dataset_name = args.dataset_name
        cfg = getattr(unet, "config", None)
        self._encode = prompt_encoder or _SeededPrompts(getattr(cfg, "ctx_len", 77), getattr(cfg, "cross_dim", 768))
        keep = lambda p: p if len(p.split(",")[0]) <= 3 else ",".join([p.split(",")[0]])      # edit.py:60-63
        self.for_prompt, self.neg_prompt, self.inv_prompt = keep(args.for_prompt), keep(args.neg_prompt), keep(args.inv_prompt)
        self.null_prompt = ""
        self.for_prompt_emb = self._get_prompt_emb(args.for_prompt)
        self.neg_prompt_emb = self._get_prompt_emb(args.neg_prompt)
        self.null_prompt_emb = self._get_prompt_emb("")
        self.inv_prompt_emb = self._get_prompt_emb(args.inv_prompt)
        self.guidance_scale = args.guidance_scale
        self.edit_prompt = args.edit_prompt
        self.edit_prompt_emb = self._get_prompt_emb(args.edit_prompt)
        self.x_edit_step_size = getattr(args, "x_edit_step_size", None)
        self.x_space_guidance_edit_step = args.x_space_guidance_edit_step
        self.x_space_guidance_scale = args.x_space_guidance_scale
        self.x_space_guidance_num_step = args.x_space_guidance_num_step
        self.x_space_guidance_use_edit_prompt = getattr(args, "x_space_guidance_use_edit_prompt", True)
        self.scheduler.set_timesteps(self.for_steps, device=self.device)
        self.edit_t = args.edit_t
        self.edit_t_idx = (self.scheduler.timesteps - self.edit_t * 1000).abs().argmin()       # edit.py:95
        self.result_folder, self.obs_folder = args.result_folder, args.obs_folder
        self.input_root = getattr(args, "input_root", "./inputs")
        self.EXP_NAME = "exp"

    def _get_prompt_emb(self, prompt):
        with T.phase("prompt encoding (CLIP text model)"):
            return self._encode(prompt).to(device=self.device, dtype=torch.float32)

    @torch.no_grad()
    def run_DDIMforward(self, num_samples=5):
        self.EXP_NAME = f"DDIMforward-for_{self.for_prompt}"
        zT = torch.randn(num_samples, self.c_in, self.image_size, self.image_size).to(device=self.device, dtype=self.dtype)
        return self.DDIMforwardsteps(zT, t_start_idx=0, t_end_idx=-1)

    @torch.no_grad()
    def run_DDIMinversion(self, idx, guidance=None, vis_traj=False):
        print("start DDIMinversion")
        self._phase = "DDIM inversion: U-Net forwards"
        self.EXP_NAME = f"DDIMinversion-{self.dataset_name}-{idx}-for_{self.for_prompt}-inv_{self.inv_prompt}"
        do_cfg = (self.guidance_scale > 1.0) & (guidance is not None)
        if not self.use_yh_custom_scheduler:
            raise ValueError("recommend to use yh custom scheduler")
        self.scheduler.set_timesteps(self.inv_steps, device=self.device, is_inversion=True)
        timesteps = self.scheduler.timesteps
        if self.dataset is not None and self.vae is not None:
            x0 = self.dataset[idx].to(self.device)
            save_image((x0 / 2 + 0.5).clamp(0, 1), os.path.join(self.result_folder, f"original_x0-{self.EXP_NAME}.png"))
            z0 = self.vae.encode(x0) * 0.18215                                                  # edit.py:144-146
        else:                                                                                  # synthetic latent (no VAE offline)
            z0 = torch.randn(1, self.c_in, self.image_size, self.image_size, generator=torch.Generator().manual_seed(int(idx)))
        latents = z0.to(device=self.device, dtype=self.dtype)
        for i, t in enumerate(timesteps):
            if i == len(timesteps) - 1:
                break
            if do_cfg:
                emb = torch.cat([self.null_prompt_emb.repeat(latents.size(0), 1, 1), self.inv_prompt_emb.repeat(latents.size(0), 1, 1)], dim=0)
                e_u, e_t = self._eps(torch.cat([latents] * 2), t, emb).chunk(2)
                noise_pred = e_u + self.guidance_scale * (e_t - e_u)
            else:
                noise_pred = self._eps(latents, t, self.inv_prompt_emb.repeat(latents.size(0), 1, 1))
            latents = self.scheduler.step(noise_pred, t, latents, eta=0).prev_sample
        return latents

    def _tangent_space_naming(self, op, block_idx, pca_rank, edit_prompt=None):
        """directory and EXP_NAME(idx, h_t) of the tangent-space files; edit_prompt sets the driver's prompt (None keeps it), as the sampling job does"""
        if edit_prompt is not None and edit_prompt != self.edit_prompt:
            self.edit_prompt = edit_prompt
            self.edit_prompt_emb = self._get_prompt_emb(self.edit_prompt)
        save_dir = os.path.join(self.input_root, f"local_encoder_pullback_stable_diffusion-dataset_{self.dataset_name}-num_steps_{self.for_steps}-pca_rank_{pca_rank}")
        return save_dir, lambda idx, ht: f'zt-{self.dataset_name}_{idx}-{ht}T-"{self.edit_prompt}"-{op}-block_{block_idx}-seed_{self.seed}'

    @torch.no_grad()
    def run_sample_encoder_local_tangent_space_zt(self, h_t, op, block_idx, pca_rank=50, num_local_basis=10, use_edit_prompt=None, edit_prompt=None,
                                                  vis_vT=True):
        """Reference: src/modules/edit.py:310-383 -- the local tangent spaces (u, s, vT) of num_local_basis latents at h_t, saved for analysis.
        h_t: a float, or a list (the loop of src/main.py:61-76 over EDIT_T_LIST in one call).  The pending (basis index, h_t) pairs -- each at its
        own (z_t, t): inversion or a Random latent, then DDIMforwardsteps to h_t -- advance together through local_encoder_pullback_batch instead
        of one call each; min_iter=10, max_iter=50, threshold 1e-3 as at edit.py:354-357 (its chunk_size only splits the reference's passes).
        Files: u- / s- / vT-<EXP_NAME>.pt, eigenvalue_spectrum-<EXP_NAME>.png and (vis_vT) vT-<EXP_NAME>.png in the basis directory of
        run_edit_local_encoder_pullback_zt (the reference's own directory and the -ver_ suffix of its EXP_NAME need attributes it never defines:
        sd_ver, scheduler_name; the after_res / after_sa suffixes belong to taps that do not exist here).  edit_prompt sets the prompt (None: the
        driver's own); use_edit_prompt, the reference's alternative, picks from caption lists that do not exist here and raises ValueError.  With a
        list h_t a basis index is inverted once per call, not once per h_t."""
        if use_edit_prompt is not None:                        # edit.py:323: exactly one of the two; the caption lists use_edit_prompt picks from do not exist here
            raise ValueError("use_edit_prompt selects from caption lists that are not available: pass edit_prompt (None keeps the driver's edit prompt)")
        if edit_prompt is not None:                                                             # edit.py:324
            self.edit_prompt = edit_prompt
            self.edit_prompt_emb = self._get_prompt_emb(self.edit_prompt)
        self.scheduler.set_timesteps(self.for_steps)
        save_dir, exp_name = self._tangent_space_naming(op, block_idx, pca_rank)
        pending = self._pending_tangent_spaces(h_t, num_local_basis, save_dir, exp_name)

        zTs = {}                                               # (a list h_t asks for the same latent once per h_t: one inversion per basis index and call)

        def make_zt(idx, ht):
            if idx not in zTs:
                zTs[idx] = self._random_latent(idx) if self.dataset_name == "Random" else self.run_DDIMinversion(idx=idx)   # edit.py:344-348
            zT = zTs[idx]
            self.scheduler.set_timesteps(self.for_steps, device=self.device)
            h_t_idx = int((self.scheduler.timesteps - ht * 1000).abs().argmin())                # edit.py:316
            if h_t_idx == 0:                                   # (DDIMforwardsteps announces its first step before it looks for the last: nothing to run)
                return zT, self.scheduler.timesteps[0]
            zt, t, _ = self.DDIMforwardsteps(zT, t_start_idx=0, t_end_idx=h_t_idx)              # edit.py:350-351
            return zt, t

        def finish(name, s, vT, lat_shape):
            self.EXP_NAME = name
            if vis_vT:
                save_vT_visualisation(vT, lat_shape, os.path.join(save_dir, f"vT-{name}.png"))  # edit.py:359-369
        self._sample_tangent_spaces(pending, make_zt, self.edit_prompt_emb, op, block_idx, pca_rank, 1e-3, save_dir, finish)

    @torch.no_grad()
    def DDIMforwardsteps(self, zt, t_start_idx, t_end_idx, **kwargs):
        print("start DDIMforward")
        self._phase = "DDIM forward to edit_t: U-Net forwards" if t_end_idx != -1 else "DDIM decode of the edited latents: U-Net forwards"
        do_cfg = self.guidance_scale > 1.0
        if not self.use_yh_custom_scheduler:
            raise ValueError("recommend to use yh custom scheduler")
        self.scheduler.set_timesteps(self.for_steps, device=self.device)
        latents = zt
        for t_idx, t in enumerate(self.scheduler.timesteps):
            if t_idx < t_start_idx:
                continue
            elif t_start_idx == t_idx:
                print("t_start_idx : ", t_idx)
            elif t_idx == t_end_idx:                                                            # edit.py:429-431
                print("t_end_idx : ", t_idx)
                return latents, t, t_idx
            outs = []
            for lat in self._chunks(latents, 2 if do_cfg else 1):
                if do_cfg:
                    emb = torch.cat([self.neg_prompt_emb.repeat(lat.size(0), 1, 1), self.for_prompt_emb.repeat(lat.size(0), 1, 1)], dim=0)
                    e_u, e_c = self._eps(torch.cat([lat] * 2, dim=0), t, emb).chunk(2)
                    noise_pred = e_u + self.guidance_scale * (e_c - e_u)
                else:
                    noise_pred = self._eps(lat, t, self.for_prompt_emb.repeat(lat.size(0), 1, 1))
                outs.append(self.scheduler.step(noise_pred, t, lat, eta=0).prev_sample)
            latents = torch.cat(outs, dim=0)
        if kwargs.get("finish", True) is False:                                                 # batched trajectories: the caller finishes each experiment
            return latents
        return self._finish_decode(latents, self.EXP_NAME)

    def _finish_decode(self, latents, exp_name):
        """edit.py:476-482: latents / 0.18215 -> VAE decode -> clamp -> one PNG row per experiment."""
        latents = 1 / 0.18215 * latents
        with T.phase("VAE decode"):
            x0 = self.vae.decode(latents) if self.vae is not None else latents
            x0 = (x0 / 2 + 0.5).clamp(0, 1) if self.vae is not None else x0
        with T.phase("image files (PNG encode + write)"):
            save_image(x0, os.path.join(self.result_folder, f"x0_gen-{exp_name}.png"), nrow=x0.size(0))
        return latents

    # run_geodesic_interpolation: the conditioning of get_h (the prompt the tangent-space job pulls back under) and the decode of the three curves
    def _geodesic_ctx(self):
        return self.edit_prompt_emb

    def _geodesic_decode(self, latents, t_idx, names):
        out = self.DDIMforwardsteps(latents, t_start_idx=t_idx, t_end_idx=-1, finish=False)
        n = out.size(0) // len(names)
        for i, name in enumerate(names):
            self._finish_decode(out[i * n:(i + 1) * n], name)

    @torch.no_grad()
    def x_space_guidance(self, zt, t_idx, vk, single_edit_step, use_edit_prompt=False):
        t = self.scheduler.timesteps[t_idx]
        self._phase = "x-space guidance: batch-2 U-Net forwards"
        zt_edit = zt + single_edit_step * vk                                                    # edit.py:490
        et = self._eps(torch.cat([zt, zt_edit], dim=0), t, self.edit_prompt_emb.repeat(2, 1, 1))
        et_null, et_edit = et.chunk(2)
        return zt + self.x_space_guidance_scale * (et_edit - et_null)                           # edit.py:501

    @torch.no_grad()
    def run_edit_local_encoder_pullback_zt(self, idx, op, block_idx, vis_num, vis_num_pc=1, vis_vT=False, pca_rank=50,
                                           edit_prompt=None, edit_t=None):
        print(f"current experiment : idx : {idx}, op : {op}, block_idx : {block_idx}, vis_num : {vis_num}, vis_num_pc : {vis_num_pc}, pca_rank : {pca_rank}, edit_prompt : {edit_prompt}")
        if edit_prompt is not None:
            self.edit_prompt = edit_prompt
            self.edit_prompt_emb = self._get_prompt_emb(self.edit_prompt)
        self.scheduler.set_timesteps(self.for_steps)
        zT = self.run_DDIMinversion(idx=idx)
        zt, t, t_idx = self.DDIMforwardsteps(zT, t_start_idx=0, t_end_idx=self.edit_t_idx)
        assert t_idx == self.edit_t_idx
        name = f'local_basis-{self.dataset_name}_{idx}-{self.edit_t}T-"{self.edit_prompt}"-{op}-block_{block_idx}-seed_{self.seed}'
        save_dir = os.path.join(self.input_root, f"local_encoder_pullback_stable_diffusion-dataset_{self.dataset_name}-num_steps_{self.for_steps}-pca_rank_{pca_rank}")
        u_path, s_path, vT_path = self._basis_paths(save_dir, name)
        if os.path.exists(u_path) and os.path.exists(vT_path):
            u = torch.load(u_path, map_location=self.device).type(self.dtype)
            vT = torch.load(vT_path, map_location=self.device).type(self.dtype)
        else:
            print("!!!RUN LOCAL PULLBACK!!!")
            with T.phase("local_encoder_pullback_zt (power iteration)"):
                u, s, vT = self.unet.local_encoder_pullback_zt(
                    sample=zt, timestep=t, encoder_hidden_states=self.edit_prompt_emb, op=op, block_idx=block_idx,
                    pca_rank=pca_rank, chunk_size=5, min_iter=10, max_iter=50, convergence_threshold=1e-4)   # edit.py:236-239
            vT = vT.to(device=self.device, dtype=self.dtype)
            torch.save(u, u_path); torch.save(s, s_path); torch.save(vT, vT_path)
            save_spectrum_plot(s, os.path.join(save_dir, f"eigenvalue_spectrum-{name}.png"))        # edit.py:249-251
            save_vT_visualisation(vT, zT.shape[1:], os.path.join(self.obs_folder, f"vT-{name}.png"))    # edit.py:253-263
        self.last_basis = (u, vT)
        u = u / u.norm(dim=0, keepdim=True)                                                     # edit.py:267-268
        vT = vT / vT.norm(dim=1, keepdim=True)
        original_zt = zt.clone()
        results = []
        if self.trajectory_batch > 1:
            return self._edit_trajectories_together(idx, op, block_idx, vis_num, vis_num_pc, vT, original_zt, zT.shape[1:])
        for pc_idx in range(vis_num_pc):
            for direction in [1, -1]:
                tag = "pos" if direction == 1 else "neg"
                self.EXP_NAME = f"Edit_zt-{self.dataset_name}_{idx}-edit_{self.edit_t}T-{op}-block_{block_idx}-pc_{pc_idx:0=3d}_{tag}-edit_prompt_{self.edit_prompt}"
                if os.path.exists(os.path.join(self.result_folder, self.EXP_NAME + ".png")):
                    print("!!!ALREADY DONE EXP!!!")
                    continue
                vk = direction * vT[pc_idx, :].view(-1, *zT.shape[1:])
                zt_list = [original_zt.clone()]
                for _ in range(self.x_space_guidance_num_step):
                    zt_list.append(self.x_space_guidance(zt_list[-1], t_idx=self.edit_t_idx, vk=vk,
                                                         single_edit_step=self.x_space_guidance_edit_step,
                                                         use_edit_prompt=self.x_space_guidance_use_edit_prompt))
                zt = torch.cat(zt_list, dim=0)
                zt = zt[::(zt.size(0) // vis_num)]                                              # edit.py:301-302
                results.append(self.DDIMforwardsteps(zt, t_start_idx=self.edit_t_idx, t_end_idx=-1))
        return results

    def _edit_trajectories_together(self, idx, op, block_idx, vis_num, vis_num_pc, vT, original_zt, lat_shape):
        """The loop body of edit.py:276-307 for all pending (pc, +-) experiments at once (self.trajectory_batch > 1): same experiments, names and skips;
        results equal to the sequential path up to 16-bit rounding (the GEMM tile / split-K selection depends on batch x rows, so a batch-2n call sums
        in another order than n batch-2 calls: fp32 engines agree to 2e-3, bf16 to a few 1e-2 over the chained steps -- tests/test_gpu_edit.py); the n chains of x-space guidance take ONE U-Net call of batch 2 n per step ([z_1..z_n | z_1 + s v_1 .. z_n + s v_n]) and the n * (vis_num + 1)
        decode trajectories ONE call of that batch per DDIM step (further split only by the engine's batch limit)."""
        todo = []
        for pc_idx in range(vis_num_pc):
            for direction in [1, -1]:
                tag = "pos" if direction == 1 else "neg"
                name = f"Edit_zt-{self.dataset_name}_{idx}-edit_{self.edit_t}T-{op}-block_{block_idx}-pc_{pc_idx:0=3d}_{tag}-edit_prompt_{self.edit_prompt}"
                if os.path.exists(os.path.join(self.result_folder, name + ".png")):
                    print("!!!ALREADY DONE EXP!!!")
                    continue
                todo.append((name, direction * vT[pc_idx, :].view(-1, *lat_shape)))
        if not todo:
            return []
        n = len(todo)
        t = self.scheduler.timesteps[self.edit_t_idx]
        self._phase = "x-space guidance: batch-2 U-Net forwards"
        vk = torch.cat([v for _, v in todo], dim=0)                                             # [n, C, H, W]
        steps = self._guidance_chains_together(original_zt.repeat(n, 1, 1, 1), vk, t, self.edit_prompt_emb)   # [n, num_step + 1, C, H, W]
        picked = steps[:, ::(steps.size(1) // vis_num)]                                         # edit.py:301-302, per chain
        m = picked.size(1)
        lat = self.DDIMforwardsteps(picked.reshape(n * m, *lat_shape), t_start_idx=self.edit_t_idx, t_end_idx=-1, finish=False)
        results = []
        for i, (name, _) in enumerate(todo):
            self.EXP_NAME = name
            results.append(self._finish_decode(lat[i * m:(i + 1) * m], name))
        return results


# =================================================================== unconditional (pixel space)
class EditUncondDiffusion(_EditBase):
    def __init__(self, args, unet=None, dataset=None):
        self.memory_bound = getattr(args, "memory_bound", 50)
        # > 1: the chains of run_edit_parallel_transport advance together (one U-Net call of 2 n rows per guidance step, one decode batch); 0 / 1: the
        # reference's order, one chain at a time.  The other jobs of this driver do not read it beyond the batch bound of _chunks.
        self.trajectory_batch = int(getattr(args, "trajectory_batch", 0) or 0)
        self.memory_bound_given = getattr(args, "memory_bound_given", None)
        self.h_t = getattr(args, "h_t", 0.8)
        self.device = torch.device(args.device)
        self.dtype = getattr(args, "dtype", torch.float32)
        self.seed = args.seed
        self.unet = unet
        self.scheduler = get_custom_diffusion_scheduler(args)
        self.model_name = args.model_name
        self.image_size = getattr(args, "image_size", 256)
        self.c_in = 3
        self.dataset = dataset
        self.dataset_name = args.dataset_name
        self.for_steps, self.inv_steps = args.for_steps, args.inv_steps
        self.use_yh_custom_scheduler = args.use_yh_custom_scheduler
        self.edit_t = args.edit_t
        self.scheduler.set_timesteps(self.for_steps, device=self.device)
        self.edit_t_idx = (self.scheduler.timesteps - self.edit_t * 1000).abs().argmin()
        pb = getattr(args, "performance_boosting_t", 0.0)
        self.performance_boosting_t_idx = (self.scheduler.timesteps - pb * 1000).abs().argmin() if pb > 0 else 1000   # edit.py:584
        self.x_space_guidance_edit_step = args.x_space_guidance_edit_step
        self.x_space_guidance_scale = args.x_space_guidance_scale
        self.x_space_guidance_num_step = args.x_space_guidance_num_step
        # "parallel-x": every chain of the global-basis jobs pushes along one x-space direction fixed at x_t (x-space guidance).  "parallel-h": the
        # h-space direction is held fixed and the x-space direction is recomputed at every state (edit.py:1202-1229; _run_parallel_h_chains)
        self.edit_xt = getattr(args, "edit_xt", "parallel-x")
        # "newton-h": every chain aims at the h-space shift h_edit_step_size along its direction by damped Gauss-Newton steps (_run_newton_h_chains)
        self.newton_iters = getattr(args, "newton_iters", 8)
        self.newton_damping = getattr(args, "newton_damping", 0.1)
        self.newton_radius = getattr(args, "newton_radius", 0.0)
        self.x_edit_step_size = getattr(args, "x_edit_step_size", 0.0)
        self.use_sega_reg = bool(getattr(args, "use_sega_reg", False))
        self.sega_reg_sigma = getattr(args, "sega_reg_sigma", 1.0)
        # "h_space_guidance" (with edit_xt at its default): the h-space direction is added at the tap at every DDIM step from edit_t down to
        # no_edit_t, scaled up to h_edit_step_size (edit.py:1232-1245; _run_h_guidance_chains); h_guidance_mode: "asyrp" or "symmetric"
        self.edit_ht = getattr(args, "edit_ht", "default")
        self.h_edit_step_size = getattr(args, "h_edit_step_size", 0.0)
        self.no_edit_t = getattr(args, "no_edit_t", 0.5)
        self.no_edit_t_idx = int((self.scheduler.timesteps - self.no_edit_t * 1000).abs().argmin())
        self.h_guidance_mode = getattr(args, "h_guidance_mode", "asyrp")
        self.result_folder, self.obs_folder = args.result_folder, args.obs_folder
        self.input_root = getattr(args, "input_root", "./inputs")
        self.EXP_NAME = "exp"

    @torch.no_grad()
    def run_DDIMforward(self, num_samples=5):
        self.EXP_NAME = "DDIMforward"
        xT = torch.randn(num_samples, self.c_in, self.image_size, self.image_size).to(device=self.device, dtype=self.dtype)
        return self.DDIMforwardsteps(xT, t_start_idx=0, t_end_idx=-1)

    @torch.no_grad()
    def run_DDIMinversion(self, idx):
        print("start DDIMinversion")
        name = f"DDIMinversion-{self.dataset_name}_{idx}"
        if not self.use_yh_custom_scheduler:
            raise ValueError("please set use_yh_custom_scheduler = True")
        self.scheduler.set_timesteps(self.inv_steps, device=self.device, is_inversion=True)
        timesteps = self.scheduler.timesteps
        if self.dataset is not None:
            x0 = self.dataset[idx]
        else:
            x0 = torch.randn(1, self.c_in, self.image_size, self.image_size, generator=torch.Generator().manual_seed(int(idx))).clamp(-1, 1)
        save_image((x0 / 2 + 0.5).clamp(0, 1), os.path.join(self.result_folder, f"original_x0-{name}.png"))
        xt = x0.to(self.device, dtype=self.dtype)
        for i, t in enumerate(timesteps):
            if i == len(timesteps) - 1:
                break
            xt = self.scheduler.step(self._eps(xt, t), t, xt, eta=0).prev_sample
        save_image((xt / 2 + 0.5).clamp(0, 1), os.path.join(self.result_folder, f"xT-{name}.png"))
        return xt

    @torch.no_grad()
    def DDIMforwardsteps(self, xt, t_start_idx, t_end_idx, vis_psd=False, save_image_=True, return_xt=True, performance_boosting=False):
        print("start DDIMforward")
        assert (t_start_idx < self.for_steps) & (t_end_idx <= self.for_steps)
        if not self.use_yh_custom_scheduler:
            raise ValueError("please set use_yh_custom_scheduler = True")
        self.scheduler.set_timesteps(self.for_steps, device=self.device)
        timesteps = self.scheduler.timesteps
        for i, t in enumerate(timesteps):
            if t_end_idx == i:                                                                  # edit.py:1640-1642
                print("t_end_idx : ", i)
                return xt, t, i
            elif i < t_start_idx:
                continue
            boost = performance_boosting & (self.performance_boosting_t_idx <= i) & (self.performance_boosting_t_idx != len(timesteps) - 1)
            eta = 1 if boost else 0                                                             # edit.py:1650-1653
            xt = torch.cat([self.scheduler.step(self._eps(c, t), t, c, eta=eta).prev_sample for c in self._chunks(xt)], dim=0)
        if save_image_:
            save_image((xt / 2 + 0.5).clamp(0, 1), os.path.join(self.result_folder, f"x0_gen-{self.EXP_NAME}.png"), nrow=xt.size(0))
        return xt if return_xt else None

    def _tangent_space_naming(self, op, block_idx, pca_rank, fix_xt=False, fix_t=False, dataset_name=None):
        """directory and EXP_NAME(idx, h_t) of the tangent-space files, -fix_xt / -fix_t appended to the directory (edit.py:1547-1550); dataset_name:
        another dataset's files (the global-basis job reads the 'Random' ones whatever dataset it edits)"""
        assert (not fix_xt) or (not fix_t)
        ds = self.dataset_name if dataset_name is None else dataset_name
        save_dir = os.path.join(self.input_root, f"local_encoder_pullback_uncond-model_{self.model_name}-dataset_{ds}-num_steps_{self.for_steps}-pca_rank_{pca_rank}")
        save_dir += "-fix_xt" if fix_xt else "-fix_t" if fix_t else ""
        return save_dir, lambda idx, ht: f"xt-{ds}_{idx}-{ht}T-{op}-block_{block_idx}-seed_{self.seed}"

    @torch.no_grad()
    def run_sample_encoder_local_tangent_space_zt(self, h_t, op, block_idx, pca_rank=50, num_local_basis=100, fix_xt=False, fix_t=False):
        """Reference: src/modules/edit.py:1517-1599 -- the local tangent spaces (u, s, vT) of num_local_basis noise images at h_t.  h_t: a float,
        or a list (the loop of src/main.py:80-91 in one call).  fix_xt pairs x = x_T with t(h_t), fix_t pairs x_t(h_t) with t = T (the two ablations
        of edit.py:1571-1576; not both).  The pending (basis index, h_t) pairs advance together through local_encoder_pullback_batch -- under
        fix_xt the rows of a group differ in t only; min_iter=10, max_iter=50, threshold 1e-4 as at edit.py:1581-1584.  Files: u- / s- /
        vT-<EXP_NAME>.pt and eigenvalue_spectrum-<EXP_NAME>.png in the basis directory of run_edit_local_encoder_pullback_zt with -fix_xt / -fix_t
        appended (the reference's own directory needs a scheduler_name it never defines)."""
        assert (not fix_xt) or (not fix_t)                                                      # edit.py:1539
        self.scheduler.set_timesteps(self.for_steps)
        save_dir, exp_name = self._tangent_space_naming(op, block_idx, pca_rank, fix_xt=fix_xt, fix_t=fix_t)
        pending = self._pending_tangent_spaces(h_t, num_local_basis, save_dir, exp_name)

        def make_xt(idx, ht):
            xT = self._random_latent(idx)                                                       # edit.py:1568: the dataset of this job holds x_T
            self.scheduler.set_timesteps(self.for_steps, device=self.device)
            h_t_idx = int((self.scheduler.timesteps - ht * 1000).abs().argmin())                # edit.py:1543
            if fix_xt:                                         # edit.py:1572-1573: x = x_T (DDIMforwardsteps(.., t_end_idx=0) returns its input), t of h_t
                return xT, self.scheduler.timesteps[h_t_idx]
            xt, t, _ = self.DDIMforwardsteps(xT, t_start_idx=0, t_end_idx=h_t_idx)
            return xt, self.scheduler.timesteps[0] if fix_t else t                              # edit.py:1575-1576
        self._sample_tangent_spaces(pending, make_xt, None, op, block_idx, pca_rank, 1e-4, save_dir, lambda name, s, vT, lat_shape: setattr(self, "EXP_NAME", name))

    # run_geodesic_interpolation: no conditioning, and the decode of the three curves as one batch (the eta = 1 tail of the other jobs' decodes)
    def _geodesic_ctx(self):
        return None

    def _geodesic_decode(self, xt, t_idx, names):
        x0 = self.DDIMforwardsteps(xt, t_start_idx=t_idx, t_end_idx=-1, save_image_=False, performance_boosting=True)
        n = x0.size(0) // len(names)
        for i, name in enumerate(names):
            save_image((x0[i * n:(i + 1) * n] / 2 + 0.5).clamp(0, 1), os.path.join(self.result_folder, f"x0_gen-{name}.png"), nrow=n)

    @torch.no_grad()
    def x_space_guidance(self, xt, t_idx, vk, single_edit_step):
        t = self.scheduler.timesteps[t_idx]
        et_null, et_edit = self._eps(torch.cat([xt, xt + single_edit_step * vk], dim=0), t).chunk(2)
        return xt + self.x_space_guidance_scale * (et_edit - et_null)

    @torch.no_grad()
    def run_edit_local_encoder_pullback_zt(self, idx, vis_num, vis_num_pc=5, pca_rank=50, op="mid", block_idx=0, **kwargs):
        if self.dataset_name == "Random":
            xT = torch.randn(1, 3, self.image_size, self.image_size).to(device=self.device, dtype=self.dtype)
        else:
            xT = self.run_DDIMinversion(idx=idx)
        xt, t, t_idx = self.DDIMforwardsteps(xT, t_start_idx=0, t_end_idx=self.edit_t_idx)
        assert t_idx == self.edit_t_idx
        name = f"local_basis-{self.dataset_name}_{idx}-{self.edit_t}T-{op}-block_{block_idx}-seed_{self.seed}"
        save_dir = os.path.join(self.input_root, f"local_encoder_pullback_uncond-model_{self.model_name}-dataset_{self.dataset_name}-num_steps_{self.for_steps}-pca_rank_{pca_rank}")
        u_path, s_path, vT_path = self._basis_paths(save_dir, name)
        if os.path.exists(u_path) and os.path.exists(vT_path):
            u = torch.load(u_path, map_location=self.device).type(self.dtype)
            vT = torch.load(vT_path, map_location=self.device).type(self.dtype)
        else:
            print("!!!RUN LOCAL PULLBACK!!!")
            u, s, vT = self.unet.local_encoder_pullback_xt(x=xt.to(device=self.device, dtype=self.dtype), t=t, op=op, block_idx=block_idx,
                                                           pca_rank=pca_rank, min_iter=10, max_iter=50, convergence_threshold=1e-4)
            torch.save(u, u_path); torch.save(vT, vT_path)
            save_spectrum_plot(s, os.path.join(save_dir, f"eigenvalue_spectrum-{name}.png"), dpi=80)   # edit.py:733-735
            save_image(vT, os.path.join(self.obs_folder, f"vT-{name}.png"))                              # edit.py:737-741 (saves the raw vT)
        self.last_basis = (u, vT)
        u = u / u.norm(dim=0, keepdim=True)
        vT = vT / vT.norm(dim=1, keepdim=True)
        original_xt = xt.detach()
        for pc_idx in range(vis_num_pc):
            for direction in [1, -1]:
                tag = "pos" if direction == 1 else "neg"
                self.EXP_NAME = f"Edit_xt-{self.dataset_name}_{idx}-edit_{self.edit_t}T-{op}-block_{block_idx}-pc_{pc_idx:0=3d}_{tag}"
                if os.path.exists(os.path.join(self.result_folder, f"x0_gen-{self.EXP_NAME}.png")):
                    print("!!!ALREADY DONE!!!")
                    continue
                vk = direction * vT[pc_idx, :].view(-1, *xt.shape[1:])
                xt_list = [original_xt.clone()]
                for _ in range(self.x_space_guidance_num_step):
                    xt_list.append(self.x_space_guidance(xt_list[-1], t_idx=self.edit_t_idx, vk=vk, single_edit_step=self.x_space_guidance_edit_step))
                xt = torch.cat(xt_list, dim=0)
                xt = xt[::(xt.size(0) // vis_num)]
                self.DDIMforwardsteps(xt, t_start_idx=self.edit_t_idx, t_end_idx=-1, performance_boosting=True)
        return xt

    def parallel_transport_plan(self, sample_idx_0, sample_idx_1, op="mid", block_idx=0, vis_num_pc=2, vis_pc_list=None, h_t=None):
        """The experiments of run_edit_parallel_transport under the reference's names (edit.py:879-881, :912-914, :944) and in its order.  Returns
        (sample_idx_0, targets, pcs, h_t, plan); plan holds per pc (runs, vk files): runs = [(EXP_NAME, target position or None, sign)] -- the
        transported pos / neg of every target, then the original pos / neg of the source, named with sample_idx_1 = sample_idx_0 -- and the
        vk-....png name of every target."""
        targets = [int(j) for j in sample_idx_1] if isinstance(sample_idx_1, (list, tuple)) else [int(sample_idx_1)]
        i0 = int(sample_idx_0)
        h_t = self.h_t if h_t is None else h_t
        pcs = list(range(vis_num_pc)) if vis_pc_list is None else [int(p) for p in vis_pc_list]
        exp = lambda j, pc, tag: (f"xt-{self.dataset_name}-sample_idx_0_{i0}-sample_idx_1_{j}-h_{h_t}T-edit_{self.edit_t}T-{op}-block_{block_idx}"
                                  f"-seed_{self.seed}-pc_{pc:0=3d}_{tag}")
        plan = []
        for pc in pcs:
            runs = [(exp(j, pc, tag), d, sign) for d, j in enumerate(targets) for sign, tag in ((1, "pos"), (-1, "neg"))]
            runs += [(exp(i0, pc, tag), None, sign) for sign, tag in ((1, "pos"), (-1, "neg"))]
            plan.append((runs, [f"vk-sample_idx_0_{i0}-sample_idx_1_{j}-pc_{pc:0=3d}.png" for j in targets]))
        return i0, targets, pcs, h_t, plan

    @torch.no_grad()
    def run_edit_parallel_transport(self, sample_idx_0, sample_idx_1, op="mid", block_idx=0, vis_num=4, vis_num_pc=2, vis_pc_list=None, pca_rank=50,
                                    h_t=None):
        """Reference: src/modules/edit.py:782-948 -- edit sample_idx_1 along the principal directions of sample_idx_0, carried over by parallel
        transport: at h_t both samples have a local basis (u, vT); component pc of the source is moved to the target as
        vk = +-normalise(Vhat_1^T (Uhat_1^T uhat_0[:, pc])) and drives x_space_guidance_num_step guidance steps from x_t(sample_idx_1) at edit_t; the
        original direction +-vhat_0[pc] does the same from x_t(sample_idx_0).  Each chain is subsampled to vis_num states and decoded into
        x0_gen-<EXP_NAME>.png; the directions [+transported, -transported, +original, -original] go to vk-....png in the obs folder.  Names and skip
        rules are the reference's (the original-direction runs carry sample_idx_1 = sample_idx_0; the job is skipped when the last pc's _neg
        picture exists, an experiment when its own does).

        sample_idx_1 may be a list of targets: one call of the transport kernel serves all of them, the original-direction chains run once and
        every target gets the reference's names (the job is skipped when every target's last picture exists).  Bases: the files of
        _tangent_space_naming(op, block_idx, pca_rank) -- what run_sample_encoder_local_tangent_space_zt writes (the reference's directory carries a
        scheduler_name it never defines) -- and the missing ones of the call are computed together by local_encoder_pullback_batch (min_iter=10,
        max_iter=50, thr=1e-4, edit.py:833-836), each at its own x_t(h_t), and saved as u- / s- / vT-.  Loaded and fresh bases alike are normalised
        (inside dpb_transport_directions); the reference normalises only what it loads.  No `pca_rank == 50` assertion.
        trajectory_batch > 1: all pending chains advance together (_guidance_chains_together) and decode in one batch; <= 1: the reference's order.
        Returns a dict: vk [D, P, N_x], coef [D, P, k], coef_norm [D, P] of the transport, pcs, targets and the EXP_NAMEs run."""
        from . import geometry
        i0, targets, pcs, h_t, plan = self.parallel_transport_plan(sample_idx_0, sample_idx_1, op, block_idx, vis_num_pc, vis_pc_list, h_t)
        picture = lambda name: os.path.exists(os.path.join(self.result_folder, f"x0_gen-{name}.png"))
        if pcs and all(picture(plan[-1][0][2 * d + 1][0]) for d in range(len(targets))):          # the last pc's _neg of every target (edit.py:789-797)
            print("!!!ALREADY DONE EXPERIMENT!!!")
            return None
        samples = list(dict.fromkeys([i0] + targets))
        xT = {i: self._random_latent(i) if self.dataset_name == "Random" else self.run_DDIMinversion(idx=i) for i in samples}      # edit.py:800-805
        self.scheduler.set_timesteps(self.for_steps, device=self.device)
        h_t_idx = int((self.scheduler.timesteps - h_t * 1000).abs().argmin())
        at_h = {i: self.DDIMforwardsteps(xT[i], t_start_idx=0, t_end_idx=h_t_idx)[:2] for i in samples}                           # edit.py:808-809

        # the local bases at h_t: the files of the sampling job; the missing ones of this call together
        save_dir, exp_name = self._tangent_space_naming(op, block_idx, pca_rank)
        files = {i: self._basis_paths(save_dir, exp_name(i, h_t)) for i in samples}
        pending = [(i, h_t, exp_name(i, h_t), files[i]) for i in samples if not (os.path.exists(files[i][0]) and os.path.exists(files[i][2]))]
        if pending:
            print("!!!RUN LOCAL PULLBACK!!!")
            self._sample_tangent_spaces(pending, lambda i, ht: at_h[i], None, op, block_idx, pca_rank, 1e-4, save_dir, lambda *a: None)
        load = lambda p: torch.load(p, map_location=self.device).to(torch.float32)
        u = {i: load(files[i][0]) for i in samples}                                             # [N_h, k] columns, as saved
        vT = {i: load(files[i][2]) for i in samples}                                            # [k, N_x] rows
        self.last_basis = (u[i0], vT[i0])

        at_edit = {i: self.DDIMforwardsteps(xT[i], t_start_idx=0, t_end_idx=self.edit_t_idx)[0].detach() for i in samples}        # edit.py:867-871
        shape = at_edit[i0].shape[1:]
        out = dict(pcs=pcs, targets=targets, names=[])
        if not pcs:
            return out
        with T.phase("parallel transport of the directions"):
            vk_t, coef, coef_norm = geometry.transport_directions(u[i0].t(), torch.stack([u[j].t() for j in targets]),
                                                                  torch.stack([vT[j] for j in targets]), pcs)
            v0 = vT[i0][pcs]
            v0 = v0 / v0.norm(dim=1, keepdim=True)                                              # edit.py:828, :923-924
        out.update(vk=vk_t, coef=coef, coef_norm=coef_norm)

        chains, pictures = [], []                              # (name, start x_t [1, ...], direction [1, ...]); (vk- file, chains shown, written after chain)
        for p, (runs, vk_files) in enumerate(plan):
            shown = [[] for _ in targets]
            for name, d, sign in runs:
                if picture(name) or any(name == c[0] for c in chains):                          # (a target equal to the source carries the original run's name)
                    print("!!!ALREADY DONE!!!")
                    continue
                for own in (shown if d is None else [shown[d]]):                                # the original directions appear in every target's vk- picture
                    own.append(len(chains))
                chains.append((name, at_edit[i0 if d is None else targets[d]], (sign * (v0[p] if d is None else vk_t[d, p])).view(1, *shape)))
            pictures += [(f, own, len(chains) - 1) for f, own in zip(vk_files, shown) if own]
        out["names"] = [c[0] for c in chains]

        def save_vk(after):                                     # edit.py:941-947: once a pc's last chain is done
            for fname, idxs, last in pictures:
                if last == after:
                    save_image(torch.cat([chains[i][2] for i in idxs], dim=0), os.path.join(self.obs_folder, fname))

        self._run_direction_chains(chains, vis_num, shape, save_vk)
        return out

    def _run_direction_chains(self, chains, vis_num, shape, after=lambda i: None):
        """chains: (EXP_NAME, start x_t [1, ...], direction [1, ...]).  Each takes x_space_guidance_num_step guidance steps at edit_t, is subsampled to
        vis_num states and decoded into x0_gen-<EXP_NAME>.png; after(i) runs once chain i's picture is written.  trajectory_batch > 1: all chains
        advance together (_guidance_chains_together) and decode in one batch; <= 1: one after another, the reference's order."""
        self._phase = "x-space guidance: batch-2 U-Net forwards"
        if self.trajectory_batch > 1 and chains:
            t = self.scheduler.timesteps[self.edit_t_idx]
            steps = self._guidance_chains_together(torch.cat([c[1] for c in chains]), torch.cat([c[2] for c in chains]), t)
            picked = steps[:, ::(steps.size(1) // vis_num)]                                     # edit.py:904, per chain
            m = picked.size(1)
            self._phase = "DDIM decode of the edited latents: U-Net forwards"
            x0 = self.DDIMforwardsteps(picked.reshape(len(chains) * m, *shape), t_start_idx=self.edit_t_idx, t_end_idx=-1, save_image_=False,
                                       performance_boosting=True)
            for i, (name, _, _) in enumerate(chains):
                self.EXP_NAME = name
                save_image((x0[i * m:(i + 1) * m] / 2 + 0.5).clamp(0, 1), os.path.join(self.result_folder, f"x0_gen-{name}.png"), nrow=m)
                after(i)
        else:
            for i, (name, start, vk) in enumerate(chains):
                self.EXP_NAME = name
                self._phase = "x-space guidance: batch-2 U-Net forwards"
                xt_list = [start.clone()]
                for _ in range(self.x_space_guidance_num_step):
                    xt_list.append(self.x_space_guidance(xt_list[-1], t_idx=self.edit_t_idx, vk=vk, single_edit_step=self.x_space_guidance_edit_step))
                xt = torch.cat(xt_list, dim=0)
                self._phase = "DDIM decode of the edited latents: U-Net forwards"
                self.DDIMforwardsteps(xt[::int(xt.size(0) / vis_num)], t_start_idx=self.edit_t_idx, t_end_idx=-1, performance_boosting=True)
                after(i)
        self._phase = _EditBase._phase

    def global_frechet_mean_paths(self, op="mid", block_idx=0, pca_rank=50, num_local_basis=100, frechet_mean_space="x", h_t=None):
        """(basis file, info file) of the global basis, in the reference's layout (edit.py:983-987; the directory without the scheduler_name the
        reference never defines): u- (space h) or v- (space x) + <h_t>T-<op>-block_<b>-seed_<seed>-num_local_basis_<n>.pt holds [N, k] columns"""
        h_t = self.h_t if h_t is None else h_t
        save_dir = os.path.join(self.input_root, f"global_frechet_mean_uncond-model_{self.model_name}-dataset_{self.dataset_name}-num_steps_{self.for_steps}-pca_rank_{pca_rank}")
        name = f"{h_t}T-{op}-block_{block_idx}-seed_{self.seed}-num_local_basis_{num_local_basis}"
        tag = "u" if frechet_mean_space == "h" else "v"
        return os.path.join(save_dir, f"{tag}-{name}.pt"), os.path.join(save_dir, f"info-{tag}-{name}.pt")

    @torch.no_grad()
    def run_edit_global_frechet_mean_zt(self, idx, op="mid", block_idx=0, vis_num=4, vis_num_pc=None, vis_pc_list=None, pca_rank=50, num_local_basis=100,
                                        local_projection=True, frechet_mean_space="x", h_t=None, frechet_max_iter=1000, frechet_tol=1e-6,
                                        frechet_init="member"):
        """Reference: src/modules/edit.py:951-1246 -- edit sample idx along the directions of a GLOBAL basis, the Frechet mean on the Grassmannian of
        num_local_basis local tangent spaces at h_t (frechet_mean_space "x": the row spans of vT; "h": the column spans of u).

        Local bases: the xt-Random_<i>-... files of the 'Random' sampling directory (what run_sample_encoder_local_tangent_space_zt writes with
        --dataset_name Random); the missing ones are computed together through _sample_tangent_spaces on seeded Gaussian latents and saved there.
        Global basis: geometry.frechet_mean (frechet_max_iter, frechet_tol; not converging is printed, not an error), rows in canonical order -- row 0
        the direction the local spaces share most -- written as [N, k] columns under global_frechet_mean_paths with an info- file (cost history,
        weight, theta, iterations) beside it; an existing file is loaded and column-normalised (edit.py:990-1003).  The reference calls a
        compute_frechet_basis it never defines (pymanopt, 10 000 iterations).
        Edit: the sample's own local basis (u, vT) at h_t is loaded or computed and saved (edit.py:1087-1133); with local_projection the global
        direction is projected on it, vk = normalise(vT^T (vT v)) for space x and normalise(vT^T (u^T u_k)) for space h (edit.py:1159-1165), both
        through geometry.transport_directions; local_projection=False uses v itself and is valid for space x only (for h the reference leaves vk
        undefined).  Then the x-space-guidance path of the driver's other jobs: chains named xt-<dataset>_<idx>-h_<h_t>T-edit_<edit_t>T-<op>-block_<b>-
        seed_<seed>-pc_<pc>_{pos,neg}, pictures x0_gen-<name>.png, projection_coeff-<name>.png in the obs folder; the job is skipped when the last
        pc's _neg picture exists, an experiment when its own does.  trajectory_batch as in run_edit_parallel_transport.
        edit_xt "parallel-h" (space h only; local_projection=False allowed): the chains of _run_parallel_h_chains instead.
        edit_ht "h_space_guidance" (space h only; local_projection=False allowed): the device DDIM chains of _run_h_guidance_chains.
        Returns a dict: basis [k, N] (rows), vk [P, N_x], pcs, names, info (None for a loaded basis).
        frechet_init "member" starts the iteration at local basis 0, "flag" at the flag mean of them all (geometry.frechet_mean(init="flag")); the
        info file of a "flag" run records it as ``init``."""
        from . import geometry
        if frechet_init not in ("member", "flag"):
            raise ValueError(f"frechet_init must be 'member' (start at local basis 0) or 'flag' (start at the flag mean), got {frechet_init!r}")
        if frechet_mean_space not in ("x", "h"):
            raise ValueError(f"frechet_mean_space must be 'x' (the spans of vT) or 'h' (the spans of u), got {frechet_mean_space!r}")
        self._check_parallel_h(frechet_mean_space)
        if frechet_mean_space == "h" and not local_projection and self.edit_xt not in ("parallel-h", "newton-h") and self.edit_ht != "h_space_guidance":
            raise ValueError("local_projection=False is valid for frechet_mean_space 'x' only: an h-space direction reaches x-space through the sample's "
                             "own local basis (the reference leaves vk undefined there)")
        h_t = self.h_t if h_t is None else h_t
        pcs = list(range(vis_num_pc or 0)) if vis_pc_list is None else [int(p) for p in vis_pc_list]
        exp = lambda pc, tag: f"xt-{self.dataset_name}_{idx}-h_{h_t}T-edit_{self.edit_t}T-{op}-block_{block_idx}-seed_{self.seed}-pc_{pc:0=3d}_{tag}"
        picture = lambda name: os.path.exists(os.path.join(self.result_folder, f"x0_gen-{name}.png"))
        if pcs and picture(exp(pcs[-1], "neg")):                                                # edit.py:971-980
            print("!!!ALREADY DONE EXP :", exp(pcs[-1], "neg"), "!!!")
            return None
        self.scheduler.set_timesteps(self.for_steps, device=self.device)
        h_t_idx = int((self.scheduler.timesteps - h_t * 1000).abs().argmin())
        load = lambda p: torch.load(p, map_location=self.device).to(torch.float32)

        # the global basis: the saved file, or the mean of the local bases
        basis_path, info_path = self.global_frechet_mean_paths(op, block_idx, pca_rank, num_local_basis, frechet_mean_space, h_t)
        os.makedirs(os.path.dirname(basis_path), exist_ok=True)
        info = None
        if os.path.exists(basis_path):
            cols = load(basis_path)
            basis = (cols / cols.norm(dim=0, keepdim=True)).t().contiguous()                    # edit.py:993, :1002
        else:
            local_dir, local_name = self._tangent_space_naming(op, block_idx, pca_rank, dataset_name="Random")
            pairs = self._tangent_space_pairs(h_t, num_local_basis, local_dir, local_name)
            pending = [p for p in pairs if not (os.path.exists(p[3][0]) and os.path.exists(p[3][2]))]    # edit.py:1020
            if pending:
                os.makedirs(local_dir, exist_ok=True)
                latent = self._random_latent if self.dataset_name == "Random" else self._seeded_latent
                self._sample_tangent_spaces(pending, lambda i, ht: self.DDIMforwardsteps(latent(i), t_start_idx=0, t_end_idx=h_t_idx)[:2], None, op,
                                            block_idx, pca_rank, 1e-4, local_dir, lambda *a: None)
            with T.phase("Frechet mean of the local bases"):
                stack = torch.stack([load(p[3][2]) if frechet_mean_space == "x" else load(p[3][0]).t() for p in pairs]).contiguous()
                basis, info = geometry.frechet_mean(stack, init="flag" if frechet_init == "flag" else 0, max_iter=frechet_max_iter, tol=frechet_tol)
                if frechet_init == "flag":
                    info["init"] = "flag"
            print(f"Frechet mean of {num_local_basis} local bases in {frechet_mean_space}-space: {info['iterations']} steps, gradient norm "
                  f"{info['grad_norm']:.3e}, cost {info['cost'][0]:.6f} -> {info['cost'][-1]:.6f}" + ("" if info["converged"] else
                  f" -- NOT converged to {frechet_tol:g} in {frechet_max_iter} steps"))
            torch.save(basis.t().contiguous().cpu(), basis_path)
            info = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in info.items()}
            torch.save(dict(info, space=frechet_mean_space, names=[p[2] for p in pairs]), info_path)

        return self._edit_along_global_basis(idx, op, block_idx, vis_num, pcs, pca_rank, h_t, frechet_mean_space, local_projection, basis,
                                             basis if frechet_mean_space == "h" else None, dict(basis=basis, pcs=pcs, names=[], info=info))

    def global_flag_mean_paths(self, op="mid", block_idx=0, pca_rank=50, num_local_basis=100, flag_mean_space="x", h_t=None, flag_rank=None,
                               flag_mean_kind="mean"):
        """(basis file, info file) of the flag-mean global basis, laid out as global_frechet_mean_paths: u- (space h) or v- (space x) +
        <h_t>T-<op>-block_<b>-seed_<seed>-num_local_basis_<n>-rank_<r>.pt holds [N, r] columns; flag_mean_kind "median": the same names with -median
        appended to the stem"""
        if flag_mean_kind not in ("mean", "median"):
            raise ValueError(f"flag_mean_kind must be 'mean' (geometry.flag_mean) or 'median' (geometry.flag_median), got {flag_mean_kind!r}")
        h_t = self.h_t if h_t is None else h_t
        r = pca_rank if not flag_rank else flag_rank
        save_dir = os.path.join(self.input_root, f"global_flag_mean_uncond-model_{self.model_name}-dataset_{self.dataset_name}-num_steps_{self.for_steps}-pca_rank_{pca_rank}")
        name = f"{h_t}T-{op}-block_{block_idx}-seed_{self.seed}-num_local_basis_{num_local_basis}-rank_{r}" + ("-median" if flag_mean_kind == "median" else "")
        tag = "u" if flag_mean_space == "h" else "v"
        return os.path.join(save_dir, f"{tag}-{name}.pt"), os.path.join(save_dir, f"info-{tag}-{name}.pt")

    @torch.no_grad()
    def run_edit_global_flag_mean_zt(self, idx, op="mid", block_idx=0, vis_num=4, vis_num_pc=None, vis_pc_list=None, pca_rank=50, num_local_basis=100,
                                     local_projection=True, flag_mean_space="x", h_t=None, flag_rank=None, flag_mean_kind="mean", flag_median_eps=1e-5,
                                     flag_median_max_rounds=50):
        """Edit sample idx along the rows of the third GLOBAL basis: the flag (extrinsic) mean of num_local_basis local tangent spaces at h_t --
        the top flag_rank eigenvectors of their mean projector (geometry.flag_mean; flag_mean_space "x": the row spans of vT, "h": the column spans of
        u).  flag_rank None or 0: pca_rank; 1 <= flag_rank <= pca_rank.  Not in the reference: where the local spaces hold a few shared directions and
        many of their own the Karcher mean of run_edit_global_frechet_mean_zt is not well posed, and the flag mean's spectrum says how many they share.

        Built like run_edit_global_frechet_mean_zt: the same xt-Random_<i>-... local-basis files of the 'Random' sampling directory, the missing ones
        sampled together and saved there; the basis written as [N, r] columns under global_flag_mean_paths with an info- file (weight, eigenvalues,
        gap, theta, iterations, converged, space, names) beside it, an existing file loaded and column-normalised; the printed summary shows the
        spectrum around row r, so that a missing gap is seen; then the common tail _edit_along_global_basis (local_projection=False: space x only).
        A pc >= flag_rank raises ValueError.  Returns a dict: basis [r, N] (rows), vk [P, N_x], pcs, names, info (None for a loaded basis).

        flag_mean_kind "median": the basis is the flag median of the same local bases (geometry.flag_median with flag_median_eps and
        flag_median_max_rounds: the L1 counterpart, on which outlying local spaces pull with a bounded force), cached under the -median names of
        global_flag_mean_paths; its info- file also holds member_weight, distance, objective and rounds, and the five members of lowest weight are
        printed by name with their distances.  "mean" is the job as it was, file names included."""
        from . import geometry
        if flag_mean_kind not in ("mean", "median"):
            raise ValueError(f"flag_mean_kind must be 'mean' (geometry.flag_mean) or 'median' (geometry.flag_median), got {flag_mean_kind!r}")
        if flag_mean_space not in ("x", "h"):
            raise ValueError(f"flag_mean_space must be 'x' (the spans of vT) or 'h' (the spans of u), got {flag_mean_space!r}")
        self._check_parallel_h(flag_mean_space)
        if flag_mean_space == "h" and not local_projection and self.edit_xt not in ("parallel-h", "newton-h") and self.edit_ht != "h_space_guidance":
            raise ValueError("local_projection=False is valid for flag_mean_space 'x' only: an h-space direction reaches x-space through the sample's "
                             "own local basis")
        r = int(pca_rank if not flag_rank else flag_rank)
        if not 1 <= r <= pca_rank:
            raise ValueError(f"flag_rank = {r} outside [1, pca_rank = {pca_rank}]")
        h_t = self.h_t if h_t is None else h_t
        pcs = list(range(vis_num_pc or 0)) if vis_pc_list is None else [int(p) for p in vis_pc_list]
        if any(p < 0 or p >= r for p in pcs):
            raise ValueError(f"the flag-mean basis has {r} rows: pcs {pcs} must lie in [0, {r})")
        exp = lambda pc, tag: f"xt-{self.dataset_name}_{idx}-h_{h_t}T-edit_{self.edit_t}T-{op}-block_{block_idx}-seed_{self.seed}-pc_{pc:0=3d}_{tag}"
        if pcs and os.path.exists(os.path.join(self.result_folder, f"x0_gen-{exp(pcs[-1], 'neg')}.png")):
            print("!!!ALREADY DONE EXP :", exp(pcs[-1], "neg"), "!!!")
            return None
        self.scheduler.set_timesteps(self.for_steps, device=self.device)
        h_t_idx = int((self.scheduler.timesteps - h_t * 1000).abs().argmin())
        load = lambda p: torch.load(p, map_location=self.device).to(torch.float32)

        median = flag_mean_kind == "median"
        basis_path, info_path = self.global_flag_mean_paths(op, block_idx, pca_rank, num_local_basis, flag_mean_space, h_t, r, flag_mean_kind)
        os.makedirs(os.path.dirname(basis_path), exist_ok=True)
        info = None
        if os.path.exists(basis_path):
            cols = load(basis_path)
            basis = (cols / cols.norm(dim=0, keepdim=True)).t().contiguous()
        else:
            local_dir, local_name = self._tangent_space_naming(op, block_idx, pca_rank, dataset_name="Random")
            pairs = self._tangent_space_pairs(h_t, num_local_basis, local_dir, local_name)
            pending = [p for p in pairs if not (os.path.exists(p[3][0]) and os.path.exists(p[3][2]))]
            if pending:
                os.makedirs(local_dir, exist_ok=True)
                latent = self._random_latent if self.dataset_name == "Random" else self._seeded_latent
                self._sample_tangent_spaces(pending, lambda i, ht: self.DDIMforwardsteps(latent(i), t_start_idx=0, t_end_idx=h_t_idx)[:2], None, op,
                                            block_idx, pca_rank, 1e-4, local_dir, lambda *a: None)
            with T.phase("flag mean of the local bases"):
                stack = torch.stack([load(p[3][2]) if flag_mean_space == "x" else load(p[3][0]).t() for p in pairs]).contiguous()
                if median:
                    basis, info = geometry.flag_median(stack, rank=r, eps=flag_median_eps, max_rounds=flag_median_max_rounds)
                else:
                    basis, info = geometry.flag_mean(stack, rank=r)
            eig = info["eigenvalues"]
            lo, hi = max(0, r - 3), min(len(eig), r + 3)
            around = " ".join(f"{v:.4f}" for v in eig[lo:r]) + " | " + " ".join(f"{v:.4f}" for v in eig[r:hi])
            if median:
                head = (f"flag median of {num_local_basis} local bases in {flag_mean_space}-space, rank {r}: {info['rounds']} rounds, objective "
                        f"{info['objective'][0]:.6f} -> {info['objective'][-1]:.6f}" + ("" if info["converged"] else " -- NOT converged")
                        + ("" if info["monotone"] else " -- NOT monotone")
                        + ("" if info["inner_converged"] else " -- an inner solve did NOT converge: row r sits inside the bulk of the spectrum"))
            else:
                head = (f"flag mean of {num_local_basis} local bases in {flag_mean_space}-space, rank {r}: {info['iterations']} iterations, residual "
                        f"{info['residual']:.3e}" + ("" if info["converged"] else " -- NOT converged: row r sits inside the bulk of the spectrum"))
            print(head
                  + f"; mean cos^2 of rows {lo} .. {hi - 1} (| after row {r - 1}): {around}"
                  + ("" if info["gap"] is None else f"; gap {info['gap']:.4f}"))
            if median:
                mw, dist = info["member_weight"].cpu(), info["distance"].cpu()
                low = torch.argsort(mw, stable=True)[:5].tolist()
                print("lowest member weights (the outlying local spaces): " + ", ".join(f"{pairs[i][2]} w={mw[i]:.3f} d={dist[i]:.3f}" for i in low))
            torch.save(basis.t().contiguous().cpu(), basis_path)
            info = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in info.items()}
            torch.save(dict(info, space=flag_mean_space, names=[p[2] for p in pairs]), info_path)

        return self._edit_along_global_basis(idx, op, block_idx, vis_num, pcs, pca_rank, h_t, flag_mean_space, local_projection, basis,
                                             basis if flag_mean_space == "h" else None, dict(basis=basis, pcs=pcs, names=[], info=info))

    def _edit_along_global_basis(self, idx, op, block_idx, vis_num, pcs, pca_rank, h_t, space, local_projection, basis, basis_h, out):
        """The common tail of the global-basis jobs (edit.py:1082-1246, :1354-1468): edit sample idx along rows pcs of `basis` [k, N] -- rows of x-space
        (space "x") or of h-space ("h").  The sample's own local basis (u, vT) at h_t is loaded or computed and saved; with local_projection
        vk = normalise(vT^T (vT v)) for x and normalise(vT^T (u^T u_k)) for h, both through geometry.transport_directions; without it (x only) v itself.
        Then the x-space-guidance chains xt-<dataset>_<idx>-h_<h_t>T-edit_<edit_t>T-<op>-block_<b>-seed_<seed>-pc_<pc>_{pos,neg}, an experiment skipped
        when its picture exists, and projection_coeff-<name>.png (its u series from rows pcs of basis_h [k, N_h], when given).  edit_xt "parallel-h"
        (space h): the same names, skip rule and order, but every chain follows its h-direction through _run_parallel_h_chains; with
        local_projection the local basis and the plot are produced as above, without it no local-basis file is read or written.  edit_ht
        "h_space_guidance" (space h): as parallel-h, with the device DDIM chains of _run_h_guidance_chains.  Fills and returns out (parallel-h and
        h_space_guidance add "chains", the chain records)."""
        from . import geometry
        exp = lambda pc, tag: f"xt-{self.dataset_name}_{idx}-h_{h_t}T-edit_{self.edit_t}T-{op}-block_{block_idx}-seed_{self.seed}-pc_{pc:0=3d}_{tag}"
        picture = lambda name: os.path.exists(os.path.join(self.result_folder, f"x0_gen-{name}.png"))
        load = lambda p: torch.load(p, map_location=self.device).to(torch.float32)
        self.scheduler.set_timesteps(self.for_steps, device=self.device)
        h_t_idx = int((self.scheduler.timesteps - h_t * 1000).abs().argmin())
        # the sample, its own local basis at h_t, its state at edit_t
        xT = self._random_latent(idx) if self.dataset_name == "Random" else self.run_DDIMinversion(idx=idx)      # edit.py:1082-1085
        own_dir, own_name = self._tangent_space_naming(op, block_idx, pca_rank)
        files = self._basis_paths(own_dir, own_name(idx, h_t))
        h_guide = self.edit_ht == "h_space_guidance"
        run_h_chains = self._run_newton_h_chains if self.edit_xt == "newton-h" else self._run_parallel_h_chains
        parallel_h = self.edit_xt in ("parallel-h", "newton-h") or h_guide    # (all follow the h-direction itself: the local basis serves the plot only)
        have = os.path.exists(files[0]) and os.path.exists(files[2]) and (local_projection or not parallel_h)   # (parallel-h reads it for the plot only)
        if local_projection and not have:
            print("!!!SAMPLE LOCAL TANGENT SPACE!!!")
            at_h = self.DDIMforwardsteps(xT, t_start_idx=0, t_end_idx=h_t_idx)[:2]
            self._sample_tangent_spaces([(idx, h_t, own_name(idx, h_t), files)], lambda i, ht: at_h, None, op, block_idx, pca_rank, 1e-4, own_dir,
                                        lambda *a: None)
            have = True
        if have:
            u, vT = load(files[0]), load(files[2])
            self.last_basis = (u, vT)
        original_xt = self.DDIMforwardsteps(xT, t_start_idx=0, t_end_idx=self.edit_t_idx)[0].detach()            # edit.py:1136-1137
        shape = original_xt.shape[1:]
        if not pcs:
            return out
        if parallel_h and not local_projection:             # edit.py:1202-1229 never reads vk: nothing of the local basis is needed
            out["vk"] = None
            chains = [(exp(pc, tag), original_xt, pc, sign) for pc in pcs for sign, tag in ((1, "pos"), (-1, "neg")) if not picture(exp(pc, tag))]
            out["names"] = [c[0] for c in chains]
            if h_guide:
                out["chains"] = self._run_h_guidance_chains([(c[0], c[2], c[3]) for c in chains], original_xt, basis, op, block_idx, vis_num, shape)
            else:
                out["chains"] = run_h_chains(chains, basis, op, block_idx, vis_num, shape)
            return out
        if local_projection:
            with T.phase("projection of the global directions on the local basis"):
                own = vT if space == "x" else u.t()
                short = own.shape[0] - basis.shape[0]            # (a basis of fewer rows than the local one: padded with row 0, which no pc beyond names)
                src = basis if short <= 0 else torch.cat([basis, basis[:1].expand(short, -1)])
                vk = geometry.transport_directions(src, own, vT, pcs)[0][0]      # [P, N_x]
        else:
            vk = basis[pcs] / basis[pcs].norm(dim=1, keepdim=True)                              # edit.py:1155-1156
        out["vk"] = vk
        chains = []
        for p, pc in enumerate(pcs):
            for sign, tag in ((1, "pos"), (-1, "neg")):
                if picture(exp(pc, tag)):                                                       # edit.py:1147-1148
                    continue
                chains.append((exp(pc, tag), original_xt, (sign * vk[p]).view(1, *shape)))
                if local_projection:
                    uk = sign * basis_h[pc] if basis_h is not None else None
                    save_projection_plot(None if uk is None else (u / u.norm(dim=0, keepdim=True)).t() @ uk,
                                         (vT / vT.norm(dim=1, keepdim=True)) @ (sign * vk[p]), os.path.join(self.obs_folder, f"projection_coeff-{exp(pc, tag)}.png"))
        out["names"] = [c[0] for c in chains]
        if parallel_h:                                       # the projection above is the plot's only: the chain follows the h-direction itself
            by_name = {exp(pc, tag): (pc, sign) for pc in pcs for sign, tag in ((1, "pos"), (-1, "neg"))}
            if h_guide:
                out["chains"] = self._run_h_guidance_chains([(c[0], *by_name[c[0]]) for c in chains], original_xt, basis, op, block_idx, vis_num, shape)
                return out
            out["chains"] = run_h_chains([(c[0], c[1], *by_name[c[0]]) for c in chains], basis, op, block_idx, vis_num, shape)
            return out
        self._run_direction_chains(chains, vis_num, shape)
        return out

    def _check_parallel_h(self, space):
        """what --edit_xt asks of a global-basis job, checked before anything is computed"""
        if self.edit_xt not in ("parallel-x", "parallel-h", "newton-h"):
            raise ValueError(f"edit_xt must be 'parallel-x', 'parallel-h' or 'newton-h', got {self.edit_xt!r}")
        self._check_h_guidance(space)
        if self.edit_xt == "newton-h":
            if space != "h":
                raise ValueError("edit_xt 'newton-h' aims at an h-space shift: it needs the h-space global basis (space 'h'), not 'x'")
            if not (float(self.h_edit_step_size) != 0 and math.isfinite(float(self.h_edit_step_size))):
                raise ValueError(f"edit_xt 'newton-h' needs h_edit_step_size != 0 (the h-space shift the chain aims at), got {self.h_edit_step_size}")
            if int(self.newton_iters) < 0 or not float(self.newton_damping) >= 0 or not float(self.newton_radius) >= 0:
                raise ValueError(f"edit_xt 'newton-h' needs newton_iters, newton_damping and newton_radius >= 0, got {self.newton_iters}, "
                                 f"{self.newton_damping}, {self.newton_radius}")
            return
        if self.edit_xt != "parallel-h":
            return
        if space != "h":
            raise ValueError("edit_xt 'parallel-h' follows an h-space direction: it needs the h-space global basis (space 'h'); for space 'x' the "
                             "reference leaves uk undefined")
        if not (float(self.x_edit_step_size) > 0):
            raise ValueError(f"edit_xt 'parallel-h' needs x_edit_step_size > 0, got {self.x_edit_step_size}")

    def _check_h_guidance(self, space):
        """what --edit_ht asks of a global-basis job, checked before anything is computed"""
        if self.edit_ht not in ("default", "h_space_guidance"):
            raise ValueError(f"edit_ht must be 'default' or 'h_space_guidance', got {self.edit_ht!r}")
        if self.edit_ht != "h_space_guidance":
            return
        if self.edit_xt in ("parallel-h", "newton-h"):
            raise ValueError(f"edit_ht 'h_space_guidance' and edit_xt {self.edit_xt!r} exclude each other: the reference takes the guidance branch with "
                             "edit_xt at its default only")
        if space != "h":
            raise ValueError("edit_ht 'h_space_guidance' adds an h-space direction at the tap: it needs the h-space global basis (space 'h'), not 'x'")
        if not (float(self.h_edit_step_size) != 0 and math.isfinite(float(self.h_edit_step_size))):
            raise ValueError(f"edit_ht 'h_space_guidance' needs h_edit_step_size != 0 (the largest scale of the ladder), got {self.h_edit_step_size}")
        if self.h_guidance_mode not in ("asyrp", "symmetric"):
            raise ValueError(f"h_guidance_mode must be 'asyrp' or 'symmetric', got {self.h_guidance_mode!r}")
        if not int(self.no_edit_t_idx) > int(self.edit_t_idx):
            raise ValueError(f"edit_ht 'h_space_guidance' needs no_edit_t_idx > edit_t_idx (no_edit_t < edit_t on the table): got step {int(self.no_edit_t_idx)} "
                             f"(no_edit_t {self.no_edit_t}) and step {int(self.edit_t_idx)} (edit_t {self.edit_t})")
        if int(self.no_edit_t_idx) > int(self.performance_boosting_t_idx):
            raise ValueError(f"edit_ht 'h_space_guidance': the guided interval (steps {int(self.edit_t_idx)} .. {int(self.no_edit_t_idx) - 1}) reaches "
                             f"performance_boosting_t_idx = {int(self.performance_boosting_t_idx)}, where the decode takes eta = 1: the chain is eta = 0 only")

    def _run_h_guidance_chains(self, exps, original_xt, basis_h, op, block_idx, vis_num, shape):
        """The h_space_guidance branch (edit.py:1232-1245, :1500-1513, whose h_space_guidance method the reference never defines).  exps: (EXP_NAME,
        pc, sign).  Every experiment runs vis_num chains from original_xt with the scales sign * linspace(0, h_edit_step_size, vis_num) along
        basis_h[pc] / ||.|| (the ladder of the x-space sibling, edit.py:1188: row 0 is the unedited reconstruction; the reference repeats one uk over
        identical rows): unet.h_space_guidance over the DDIM steps edit_t_idx .. no_edit_t_idx - 1 (t the timestep, not the index), then the plain
        decode from no_edit_t_idx into x0_gen-<EXP_NAME>.png.  Each writes hguide-<EXP_NAME>.pt into the obs folder (delta_norm, dx_norm [vis_num,
        steps], scales, timesteps, mode, states_end: the latents at no_edit_t) and prints one line.  trajectory_batch > 1: all pending chains
        through calls of at most max_batch // 2 chains and one decode batch; <= 1: one experiment after another.  Returns the records, in order."""
        if not exps:
            return []
        self.scheduler.set_timesteps(self.for_steps, device=self.device)
        ts, al, an = self.scheduler.ddim_triples(int(self.edit_t_idx), int(self.no_edit_t_idx))
        uhat = (basis_h / basis_h.norm(dim=1, keepdim=True)).t().contiguous()                   # [N_h, k]: column pc is direction pc
        ladder = torch.linspace(0, float(self.h_edit_step_size), vis_num)

        def run(group):
            self._phase = "h-space guidance chain: one grouped pass (plain + shifted rows) per DDIM step"
            n = len(group) * vis_num
            r = self.unet.h_space_guidance(x=original_xt.expand(n, *shape).to(device=self.device, dtype=self.dtype), timesteps=ts, alphas=al,
                                           alphas_next=an, u=uhat, dirs=[c[1] for c in group for _ in range(vis_num)],
                                           scales=[float(c[2]) * float(a) for c in group for a in ladder], mode=self.h_guidance_mode, op=op,
                                           block_idx=block_idx)
            end = r["states"][:, -1]
            self._phase = "DDIM decode of the edited latents: U-Net forwards"
            x0 = self.DDIMforwardsteps(end, t_start_idx=int(self.no_edit_t_idx), t_end_idx=-1, save_image_=False, performance_boosting=True)
            recs = []
            for i, c in enumerate(group):
                self.EXP_NAME = c[0]
                sl = slice(i * vis_num, (i + 1) * vis_num)
                save_image((x0[sl] / 2 + 0.5).clamp(0, 1), os.path.join(self.result_folder, f"x0_gen-{c[0]}.png"), nrow=vis_num)
                rec = {"delta_norm": r["delta_norm"][sl].cpu(), "dx_norm": r["dx_norm"][sl].cpu(), "scales": float(c[2]) * ladder,
                       "timesteps": torch.tensor(ts), "mode": self.h_guidance_mode, "states_end": end[sl].cpu()}
                torch.save(rec, os.path.join(self.obs_folder, f"hguide-{c[0]}.pt"))
                print(f"h-space guidance {c[0]} ({self.h_guidance_mode}): {len(ts)} steps t = {ts[0]:g} .. {ts[-1]:g}, scales up to "
                      f"{float(rec['scales'][-1]):g}, ||e_s - e|| {float(rec['delta_norm'][-1, 0]):.4g} -> {float(rec['delta_norm'][-1, -1]):.4g}, "
                      f"distance from the plain step, summed {float(rec['dx_norm'][-1].sum()):.4g}")
                recs.append(rec)
            return recs

        groups = [exps] if self.trajectory_batch > 1 else [[c] for c in exps]
        recs = [rec for g in groups for rec in run(g)]
        self._phase = _EditBase._phase
        return recs

    def _run_parallel_h_chains(self, chains, basis_h, op, block_idx, vis_num, shape):
        """The parallel-h branch (edit.py:1202-1229, :1470-1497).  chains: (EXP_NAME, start x_t [1, ...], pc, sign).  Each holds uk = sign *
        basis_h[pc] / ||.|| fixed and takes vis_num steps x <- x + (x_edit_step_size / vis_num) * inv_jac_xt(x, t, uk) from its start at the timestep
        timesteps[edit_t_idx] (the reference passes the INDEX edit_t_idx as t: not reproduced), with the SEGA rule when use_sega_reg; the states
        xt[::int((vis_num + 1) / vis_num)] are decoded into x0_gen-<EXP_NAME>.png.  Each chain writes chain-<EXP_NAME>.pt into the obs folder (norm,
        h_shift, h_dist, sega_std, sega_kept: one entry per step, the shifts one per state) and prints one line.  trajectory_batch > 1: all chains
        through one unet.inv_jac_chain call and one decode batch; <= 1: one after another.  Returns the chain records, in order."""
        if not chains:
            return []
        t = self.scheduler.timesteps[self.edit_t_idx]
        uhat = (basis_h / basis_h.norm(dim=1, keepdim=True)).t().contiguous()                   # [N_h, k]: column pc is direction pc (edit.py:1152-1153)
        sigma = float(self.sega_reg_sigma) if self.use_sega_reg else None
        step = float(self.x_edit_step_size) / vis_num
        stride = int((vis_num + 1) / vis_num)                                                   # edit.py:1218

        def run(group):
            self._phase = "parallel-h chain: one primal and one adjoint pass per step"
            r = self.unet.inv_jac_chain(x=torch.cat([c[1] for c in group]).to(device=self.device, dtype=self.dtype), t=t, u=uhat,
                                        dirs=[c[2] for c in group], signs=[float(c[3]) for c in group], steps=vis_num, step_size=step,
                                        sega_sigma=sigma, op=op, block_idx=block_idx)
            picked = r["states"][:, ::stride]
            m = picked.size(1)
            self._phase = "DDIM decode of the edited latents: U-Net forwards"
            x0 = self.DDIMforwardsteps(picked.reshape(len(group) * m, *shape), t_start_idx=self.edit_t_idx, t_end_idx=-1, save_image_=False,
                                       performance_boosting=True)
            recs = []
            for i, c in enumerate(group):
                self.EXP_NAME = c[0]
                save_image((x0[i * m:(i + 1) * m] / 2 + 0.5).clamp(0, 1), os.path.join(self.result_folder, f"x0_gen-{c[0]}.png"), nrow=m)
                rec = {k: r[k][i].cpu() for k in ("norm", "h_shift", "h_dist", "sega_std", "sega_kept")}
                torch.save(rec, os.path.join(self.obs_folder, f"chain-{c[0]}.pt"))
                print(f"parallel-h chain {c[0]}: {vis_num} steps of {step:g}, ||J^T u|| {float(rec['norm'][0]):.4g} -> {float(rec['norm'][-1]):.4g}, "
                      f"h shift along u {float(rec['h_shift'][-1]):.4g}, |h - h0| {float(rec['h_dist'][-1]):.4g}"
                      + (f", SEGA kept {int(rec['sega_kept'][-1])} elements" if sigma else ""))
                recs.append(rec)
            return recs

        groups = [chains] if self.trajectory_batch > 1 else [[c] for c in chains]
        recs = [rec for g in groups for rec in run(g)]
        self._phase = _EditBase._phase
        return recs

    def _run_newton_h_chains(self, chains, basis_h, op, block_idx, vis_num, shape):
        """The newton-h branch, beside _run_parallel_h_chains.  chains: (EXP_NAME, start x_t [1, ...], pc, sign).  Each aims at the h-space shift
        h_edit_step_size along uk = sign * basis_h[pc] / ||.|| in vis_num damped Gauss-Newton steps from its start, at the timestep
        timesteps[edit_t_idx] (unet.newton_h_chain: newton_iters CGLS iterations per step with newton_damping, a step's length in x clamped to
        newton_radius when that is > 0); the states picked as the sibling picks them are decoded into x0_gen-<EXP_NAME>.png.  A pos chain moves h
        ALONG uk, where parallel-h moves against it.  Each chain writes newton-<EXP_NAME>.pt into the obs folder (h_shift, h_dist, h_off: one entry
        per state; resid_norm, delta_norm, clip, inner_iterations: one per step; scale) and prints one line.  trajectory_batch > 1: all chains
        through one unet.newton_h_chain call and one decode batch; <= 1: one after another.  Returns the chain records, in order."""
        if not chains:
            return []
        t = self.scheduler.timesteps[self.edit_t_idx]
        uhat = (basis_h / basis_h.norm(dim=1, keepdim=True)).t().contiguous()                   # [N_h, k]: column pc is direction pc
        scale = float(self.h_edit_step_size)
        stride = int((vis_num + 1) / vis_num)
        keys = ("h_shift", "h_dist", "h_off", "resid_norm", "delta_norm", "clip", "inner_iterations")

        def run(group):
            self._phase = "newton-h chain: one primal pass and the inner solve's tangent and adjoint passes per step"
            r = self.unet.newton_h_chain(x=torch.cat([c[1] for c in group]).to(device=self.device, dtype=self.dtype), t=t, u=uhat,
                                         dirs=[c[2] for c in group], signs=[float(c[3]) for c in group], scale=scale, steps=vis_num,
                                         iters=int(self.newton_iters), damping=float(self.newton_damping),
                                         radius=float(self.newton_radius) or None, op=op, block_idx=block_idx)
            picked = r["states"][:, ::stride]
            m = picked.size(1)
            self._phase = "DDIM decode of the edited latents: U-Net forwards"
            x0 = self.DDIMforwardsteps(picked.reshape(len(group) * m, *shape), t_start_idx=self.edit_t_idx, t_end_idx=-1, save_image_=False,
                                       performance_boosting=True)
            recs = []
            for i, c in enumerate(group):
                self.EXP_NAME = c[0]
                save_image((x0[i * m:(i + 1) * m] / 2 + 0.5).clamp(0, 1), os.path.join(self.result_folder, f"x0_gen-{c[0]}.png"), nrow=m)
                rec = {k: r[k][i].cpu() for k in keys}
                rec["scale"] = scale
                torch.save(rec, os.path.join(self.obs_folder, f"newton-{c[0]}.pt"))
                print(f"newton-h chain {c[0]}: {vis_num} steps of {int(self.newton_iters)} iterations, h shift along u {float(rec['h_shift'][-1]):.4g} "
                      f"of {scale:g} asked, off-axis {float(rec['h_off'][-1]):.4g}, inner iterations {[int(a) for a in rec['inner_iterations']]}")
                recs.append(rec)
            return recs

        groups = [chains] if self.trajectory_batch > 1 else [[c] for c in chains]
        recs = [rec for g in groups for rec in run(g)]
        self._phase = _EditBase._phase
        return recs

    def global_hungarian_mean_paths(self, op="mid", block_idx=0, pca_rank=50, h_t=None):
        """{"u": (basis file, info file), "v": ...} of the two Hungarian global bases, in the reference's layout (edit.py:1270-1274; the directory
        without the scheduler_name the reference never defines): {u,v}-<h_t>T-<op>-block_<b>-seed_<seed>.pt holds [N, k] columns.  The reference's
        name does not carry num_local_basis; the info- file beside it does."""
        h_t = self.h_t if h_t is None else h_t
        save_dir = os.path.join(self.input_root, f"global_hungarian_mean_uncond-model_{self.model_name}-dataset_{self.dataset_name}-num_steps_{self.for_steps}-pca_rank_{pca_rank}")
        name = f"{h_t}T-{op}-block_{block_idx}-seed_{self.seed}"
        return {tag: (os.path.join(save_dir, f"{tag}-{name}.pt"), os.path.join(save_dir, f"info-{tag}-{name}.pt")) for tag in ("u", "v")}

    @torch.no_grad()
    def run_edit_global_hungarian_mean_zt(self, idx, op="mid", block_idx=0, vis_num=4, vis_num_pc=None, vis_pc_list=None, pca_rank=50, num_local_basis=100,
                                          local_projection=True, hungarian_mean_space="x", h_t=None, hungarian_distance="1/cosine",
                                          hungarian_max_sweeps=20):
        """Reference: src/modules/edit.py:1249-1514 -- edit sample idx along the directions of the other GLOBAL basis, the Hungarian-matched mean of
        num_local_basis local tangent spaces at h_t: the k singular directions of every local basis are matched one to one, and sign by sign, to those
        of local basis 0, and the matched unit vectors are averaged (geometry.hungarian_mean; hungarian_distance '1/cosine' is the reference's call,
        hungarian_max_sweeps re-matches against the mean until nothing changes).  "Direction 3" then means the same thing at every sample, where the
        rows of the Frechet basis are canonical only up to an eigen-ordering.  The reference calls a compute_hungarian_basis it never defines.

        Local bases: the xt-Random_<i>-... files of the 'Random' sampling directory; the missing ones are sampled together, as in
        run_edit_global_frechet_mean_zt.  Global bases: BOTH are computed, as the reference does -- u- from the stack of u^T, v- from the stack of vT --
        and written as [N, k] columns under global_hungarian_mean_paths, each with an info- file (perm, sign, cost, weight, names, num_local_basis,
        distance, sweeps, converged).  An existing file is loaded and normalised, u by column and v as edit.py:1282-1283 does (along dim 1 of the
        [N, k] file); an info- file that records another num_local_basis or distance raises ValueError (no info- file: a reference-written cache,
        loaded as is).  The reference's v load branch reloads u (edit.py:1350-1352): not reproduced.
        Edit: the common tail of the global-basis jobs (_edit_along_global_basis).  hungarian_mean_space "x": vk = normalise(vT^T (vT vhat_pc)), the
        reference's live path; "h": vk = normalise(vT^T (u^T uhat_pc)), the route the Frechet job uses to bring an h-direction to x.
        local_projection=False is valid for "x" only -- and for edit_xt "parallel-h" (space h only), whose chains are those of
        _run_parallel_h_chains -- and for edit_ht "h_space_guidance" (space h only), the device DDIM chains of _run_h_guidance_chains.
        Returns a dict: basis_u [k, N_h], basis_v [k, N_x] (rows), vk [P, N_x], pcs, names, info ({"u": ..., "v": ...}, None for a loaded basis)."""
        from . import geometry
        if hungarian_mean_space not in ("x", "h"):
            raise ValueError(f"hungarian_mean_space must be 'x' (the directions of vT) or 'h' (the directions of u), got {hungarian_mean_space!r}")
        self._check_parallel_h(hungarian_mean_space)
        if hungarian_mean_space == "h" and not local_projection and self.edit_xt not in ("parallel-h", "newton-h") and self.edit_ht != "h_space_guidance":
            raise ValueError("local_projection=False is valid for hungarian_mean_space 'x' only: an h-space direction reaches x-space through the "
                             "sample's own local basis")
        if hungarian_distance not in geometry.HUNGARIAN_DISTANCES:
            raise ValueError(f"hungarian_distance must be one of {sorted(geometry.HUNGARIAN_DISTANCES)}, got {hungarian_distance!r}")
        h_t = self.h_t if h_t is None else h_t
        pcs = list(range(vis_num_pc or 0)) if vis_pc_list is None else [int(p) for p in vis_pc_list]
        exp = lambda pc, tag: f"xt-{self.dataset_name}_{idx}-h_{h_t}T-edit_{self.edit_t}T-{op}-block_{block_idx}-seed_{self.seed}-pc_{pc:0=3d}_{tag}"
        if pcs and os.path.exists(os.path.join(self.result_folder, f"x0_gen-{exp(pcs[-1], 'neg')}.png")):
            print("!!!ALREADY DONE EXP :", exp(pcs[-1], "neg"), "!!!")
            return None
        self.scheduler.set_timesteps(self.for_steps, device=self.device)
        h_t_idx = int((self.scheduler.timesteps - h_t * 1000).abs().argmin())
        load = lambda p: torch.load(p, map_location=self.device).to(torch.float32)

        paths = self.global_hungarian_mean_paths(op, block_idx, pca_rank, h_t)
        os.makedirs(os.path.dirname(paths["u"][0]), exist_ok=True)
        bases, infos = {}, {"u": None, "v": None}
        for tag, (basis_path, info_path) in paths.items():
            if not os.path.exists(basis_path):
                continue
            if os.path.exists(info_path):
                rec = torch.load(info_path, weights_only=False)
                if rec.get("num_local_basis") != num_local_basis or rec.get("distance") != hungarian_distance:
                    raise ValueError(f"{info_path} records num_local_basis = {rec.get('num_local_basis')}, distance = {rec.get('distance')!r}; asked for "
                                     f"{num_local_basis}, {hungarian_distance!r} (the basis file's name does not carry them: move it away to recompute)")
            cols = load(basis_path)
            cols = cols / cols.norm(dim=0 if tag == "u" else 1, keepdim=True)                   # edit.py:1282-1283
            bases[tag] = cols.t().contiguous()
        if len(bases) < 2:
            local_dir, local_name = self._tangent_space_naming(op, block_idx, pca_rank, dataset_name="Random")
            pairs = self._tangent_space_pairs(h_t, num_local_basis, local_dir, local_name)
            pending = [p for p in pairs if not (os.path.exists(p[3][0]) and os.path.exists(p[3][2]))]    # edit.py:1298
            if pending:
                os.makedirs(local_dir, exist_ok=True)
                latent = self._random_latent if self.dataset_name == "Random" else self._seeded_latent
                self._sample_tangent_spaces(pending, lambda i, ht: self.DDIMforwardsteps(latent(i), t_start_idx=0, t_end_idx=h_t_idx)[:2], None, op,
                                            block_idx, pca_rank, 1e-4, local_dir, lambda *a: None)
            for tag in ("u", "v"):
                if tag in bases:
                    continue
                with T.phase("Hungarian mean of the local bases"):
                    stack = torch.stack([load(p[3][0]).t() if tag == "u" else load(p[3][2]) for p in pairs]).contiguous()
                    basis, info = geometry.hungarian_mean(stack, init=0, distance=hungarian_distance, max_sweeps=hungarian_max_sweeps)   # edit.py:1339, :1347
                print(f"Hungarian mean ({tag}) of {num_local_basis} local bases: {info['sweeps']} sweeps, changed {info['changed']}, mean weight "
                      f"{float(info['weight'].mean()):.4f}" + ("" if info["converged"] else f" -- NOT converged in {hungarian_max_sweeps} sweeps"))
                torch.save(basis.t().contiguous().cpu(), paths[tag][0])
                info = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in info.items()}
                info.update(names=[p[2] for p in pairs], num_local_basis=num_local_basis)
                torch.save(info, paths[tag][1])
                bases[tag], infos[tag] = basis, info
        use = "u" if hungarian_mean_space == "h" else "v"
        out = dict(basis_u=bases["u"], basis_v=bases["v"], pcs=pcs, names=[], info=infos if (infos["u"] or infos["v"]) else None)
        return self._edit_along_global_basis(idx, op, block_idx, vis_num, pcs, pca_rank, h_t, hungarian_mean_space, local_projection, bases[use],
                                             bases["u"], out)
