"""Host-side mirror of the reference's U-Net plugin surface for the pullback path.

Three network kinds: "sd" (diffusers UNet2DConditionModel), "ddpm" (the vendored PullBackDDPM) and "adm" (the vendored guided-diffusion
UNetModel, src/models/guided_diffusion/unet.py:398-781, which has the x= / t= surface of the DDPM kind).

The reference attaches ``get_h`` / ``local_encoder_pullback_zt`` (Stable Diffusion) and
``get_h`` / ``local_encoder_pullback_xt`` (unconditional) onto a diffusers U-Net with
``types.MethodType`` (reference src/utils/utils.py:103-104, :326-337).  ``PullbackUNet`` is a
U-Net object exposing exactly those methods (same names, argument meaning, return layout and
error behaviour) on top of the HIP engine; ``bind`` attaches them onto an existing module.

Semantics kept from the reference (src/utils/utils.py:722-816 and :165-249):
  * returns ``u`` [N_h, k] as a transposed (non-contiguous) view whose columns are J V_prev of
    the last iteration (un-normalised), ``s`` = sqrt(singular values of J^T J V_prev), ``vT`` [k, N_in];
  * stop iff allclose(V_prev, V, atol=thr, rtol=1e-5) and i > min_iter, at most max_iter iterations;
  * prints the per-iteration ``torch.dist(V_prev, V)`` and the runtime like the reference;
  * invalid (op, block_idx) raises ValueError with the reference's message (utils.py:527).
Deliberate differences:
  * the primal forward runs once per call (x_t, t fixed) instead of inside every JVP/VJP;
  * all k tangents ride one batched pass; ``chunk_size`` is accepted and only bounds the batch;
  * V0 is drawn on the CPU generator (reproducible; the reference's device RNG draw is not) or injected;
  * each singular vector is signed for non-negative overlap with the previous iterate (LAPACK's
    sign is arbitrary), which only makes the reference's stop rule well defined;
  * pca_rank <= 128 (RANK_LIMIT: the k x k eigen-solve of the re-orthonormalisation lives in LDS; the reference's signature default is 50, its
    call sites use 2..10: main.py:33, BASELINE configs); an engine is built for `max_rank` tangents (default 56).
"""
from __future__ import annotations

import math
import time
import types
from typing import Optional, Tuple

import torch

from . import lib as L
from .engine import Engine, pca_lowrank
from .engine import timesteps as _timesteps
from .tape import build_adm, build_ddpm, build_sd

MAX_RANK = 56          # default tangent capacity of an engine (workspace sizing)
RANK_LIMIT = 128       # largest pca_rank of the library (csrc/kernels.h ORTH_MAX_RANK)


class UNetOutput:
    """Mirror of diffusers' UNet2DConditionOutput: the reference reads ``.sample`` (edit.py:454-458)."""

    def __init__(self, sample):
        self.sample = sample


def _t_shared(t, batch: int, what: str) -> float:
    """the timestep of a call that takes ONE for its batch: engine.timesteps' rule, and distinct per-sample timesteps are refused by name"""
    v = t.reshape(-1).tolist() if torch.is_tensor(t) else list(t) if isinstance(t, (list, tuple)) else [t]
    if len(set(float(a) for a in v)) > 1:                  # whatever the batch: several timesteps are what this call cannot take
        raise ValueError(f"{what} takes one timestep for its batch, got {len(v)} with distinct values: per-sample timesteps are honoured by get_h, the "
                         "U-Net call, pullback_fixed, decoder_pullback_fixed, global_pca_zt and local_encoder_pullback_batch only")
    return _timesteps(t, batch)                            # (equal entries: one timestep, if there is one or one per sample)


def _conv_finite(what: str, i: int, conv, batch: bool = False) -> None:
    """The power iterations' guard: conv [B][2] as read back at iteration i (0-based) must be finite.  dpb_orth answers a NaN or an inf in W = J^T J V
    (an fp16 tangent that overflowed) or in V_prev with conv = (NaN, NaN) and a NaN basis (include/dpb.h): that iteration is never counted as
    converged -- the reference's svd raises on such input and its allclose is False on NaN."""
    bad = [b for b, c in enumerate(conv) if not all(math.isfinite(float(a)) for a in c)]
    if bad:
        where = f" for sample(s) {bad} of the batch" if batch else ""
        raise L.DpbError(f"{what}: the convergence figures of iteration {i} are not finite{where} (conv = {[list(conv[b]) for b in bad]}): W = J^T J V "
                         "or V_prev holds a NaN or an inf, e.g. an fp16 tangent that overflowed; the basis of this iteration is NaN")


class PullbackUNet:
    def __init__(self, kind: str, cfg, params, dtype=torch.float32, device="cuda:0", max_batch: int = 5,
                 max_rank: int = MAX_RANK, upto: Optional[Tuple[str, int]] = None, verbose: bool = True):
        if kind not in ("sd", "ddpm", "adm"):
            raise ValueError(f"unknown network kind {kind!r}: 'sd' (diffusers UNet2DConditionModel), 'ddpm' (vendored PullBackDDPM) or 'adm' "
                             "(guided-diffusion UNetModel)")
        self.kind, self.config, self.dtype_compute = kind, cfg, dtype
        self.device = torch.device(device)
        self.dtype = torch.float32                       # boundary dtype (what callers see)
        self.verbose = verbose
        if kind == "sd":
            tape = build_sd(cfg, params, dtype, self.device, upto)
            self.engine = Engine(tape, cfg.block_out_channels[0], True, False, cfg.in_channels, max_batch, max_rank)
            self.in_shape = (cfg.in_channels, cfg.sample_size, cfg.sample_size)
        elif kind == "adm":
            # guided-diffusion's timestep_embedding (nn.py): [cos | sin], exponent denominator half -- the SD form of the sinusoid
            tape = build_adm(cfg, params, dtype, self.device, upto)
            self.engine = Engine(tape, cfg.model_channels, True, False, cfg.in_channels, max_batch, max_rank)
            self.in_shape = (cfg.in_channels, cfg.image_size, cfg.image_size)
        else:
            tape = build_ddpm(cfg, params, dtype, self.device, upto)
            self.engine = Engine(tape, cfg.ch, False, True, cfg.in_channels, max_batch, max_rank)
            self.in_shape = (cfg.in_channels, cfg.resolution, cfg.resolution)
        self.max_rank = max_rank
        # False: local_encoder_pullback_zt / _xt run all k directions here (default).  None or a torch.distributed group: the directions of the
        # ONE sample are dealt to that group's ranks (every rank must make the same call; see _pullback and dist.k_sharded_power_iteration)
        self.k_shard_group = False

    # ------------------------------------------------------------------ feature map
    def _tap(self, op, block_idx):
        if self.kind == "adm" and op is None and block_idx is None:
            op, block_idx = "mid", 0                      # UNetModel.get_h takes no (op, block_idx): it is the middle block's output (unet.py:686-702)
        key = (op, block_idx)
        if key not in self.engine.tape.taps:
            raise ValueError(f"(op, block_idx) = ({op, block_idx}) is not valid")
        return key

    def get_h(self, sample=None, timestep=None, encoder_hidden_states=None, op=None, block_idx=None, verbose=False,
              x=None, t=None, **kwargs):
        """SD: get_h(sample, timestep, encoder_hidden_states, op, block_idx) (utils.py:438-441);
        uncond: get_h(x, t, op, block_idx) (utils.py:114-116).  Returns [B, C, H, W] features."""
        sample = x if sample is None else sample
        timestep = t if timestep is None else timestep
        key = self._tap(op, block_idx)
        h = self.engine.forward(sample, timestep, encoder_hidden_states, key)       # a timestep per sample is honoured (engine.timesteps)
        if verbose:
            print(f"op : {op}, block_idx : {block_idx}, return h.shape : {h.shape}")
        return h.to(sample.dtype)

    def __call__(self, sample, timestep, encoder_hidden_states=None, **kwargs):
        """The U-Net itself.  uncond: PullBackDDPM.forward(x, t, u=None, op=None, block_idx=None) (diffusion.py:145-200) -- with u, eps of
        the net with u added to the activation at (op, block_idx); SD: unet(sample, timestep, encoder_hidden_states).sample, whose shifted
        form is forward_dh (a u= / uk= here raises instead of being dropped).  Without u / op / block_idx: the plain forward pass."""
        shift = {k: kwargs[k] for k in ("u", "uk", "op", "block_idx") if kwargs.get(k) is not None}
        if shift:
            if self.kind == "sd":
                raise TypeError("the SD U-Net call takes no h-space shift (" + ", ".join(shift) + " given): use "
                                "forward_dh(sample, timestep, encoder_hidden_states, op=, block_idx=, uk=)")
            if "uk" in shift:
                raise TypeError("the DDPM forward takes the shift as u= (uk= is forward_dh's name for it)")
            return self._forward_shifted(sample, timestep, None, shift.get("u"), shift.get("op"), shift.get("block_idx"))
        eps = self.engine.forward(sample, timestep, encoder_hidden_states, "eps").to(sample.dtype)
        return UNetOutput(eps) if self.kind == "sd" else eps

    # ------------------------------------------------------------------ h-space shift: the forward pass with h + u at the tap
    def _forward_shifted(self, sample, timestep, ctx, u, op, block_idx):
        """eps with u.view(-1, C, H, W) added at the tap (op, block_idx): one row is broadcast over the batch, B rows give one per sample"""
        if u is None or op is None or block_idx is None:
            raise ValueError("an h-space shift needs all of u, op and block_idx")
        key = self._decoder_tap(op, block_idx)
        b, d = sample.shape[0], self.engine.tap_numel(key)
        if u.numel() == 0 or u.numel() % d:
            raise ValueError(f"u has {u.numel()} elements, the tap ({op}, {block_idx}) has {d}")
        rows = u.numel() // d
        if rows not in (1, b):
            raise ValueError(f"u holds {rows} shifts of the tap for a batch of {b}: 1 (broadcast) or one per sample")
        dirs = [0] * b if rows == 1 else list(range(b))
        e = self.engine.forward_shift(sample, _t_shared(timestep, b, "the h-space shifted forward (forward_dh, unet(x, t, u=...))"), ctx, key,
                                      u.reshape(rows, d), dirs, [1.0] * b, "eps")
        return e.to(sample.dtype)

    def forward_dh(self, sample=None, timestep=None, encoder_hidden_states=None, cross_attention_kwargs=None, op=None, block_idx=None, uk=None,
                   verbose=False):
        """Reference: utils.forward_dh, src/utils/utils.py:350-436 (SD): the eps TENSOR (not an output object) of the U-Net with
        uk.view(-1, C, H, W) added to the activation at (op, block_idx) -- 'down' (after the block's downsampler; the last skip of the block is
        that same tensor and is shifted with it), 'mid', 'up'.  The after_res / after_sa sub-block taps, which the reference names and never
        defines, do not exist here.  Without op and uk: the plain eps."""
        if self.kind != "sd":
            raise TypeError("forward_dh is the SD form; the DDPM net takes unet(x, t, u=, op=, block_idx=)")
        if op is None and block_idx is None and uk is None:
            return self.engine.forward(sample, _t_shared(timestep, sample.shape[0], "forward_dh"), encoder_hidden_states, "eps").to(sample.dtype)
        e = self._forward_shifted(sample, timestep, encoder_hidden_states, uk, op, block_idx)
        if verbose:
            print(f"op : {op}, block_idx : {block_idx}, return eps.shape : {tuple(e.shape)}")
        return e

    def h_traversal(self, x, t, ctx, u, scales, op, block_idx, pcs=None):
        """eps [len(pcs), len(scales), C, H, W] of ONE sample x [1, ...] moved along h-space directions: entry (i, j) is the net with
        scales[j] * u[:, pcs[i]] / ||u[:, pcs[i]]|| added at the tap (op, block_idx).  u [D, k] as the pullbacks and PCAs return it (columns;
        pcs=None: all of them).  The rows go through shared-prefix calls of at most max_batch: the part of the net up to the tap runs once per
        call, the directions are uploaded once and addressed per row."""
        if x.shape[0] != 1:
            raise ValueError("h_traversal moves a single sample (batch 1)")
        key = self._decoder_tap(op, block_idx)
        eng = self.engine
        d = eng.tap_numel(key)
        if u.dim() != 2 or u.shape[0] != d:
            raise ValueError(f"u must be [{d}, k] (columns: directions at the tap ({op}, {block_idx})), got {tuple(u.shape)}")
        pcs = list(range(u.shape[1])) if pcs is None else [int(i) for i in pcs]
        scales = [float(a) for a in scales]
        if not pcs or not scales or min(pcs) < 0 or max(pcs) >= u.shape[1]:
            raise ValueError(f"pcs must be a non-empty subset of range({u.shape[1]}) and scales non-empty")
        U = u.detach().to(device=self.device, dtype=torch.float32)
        U = (U / U.norm(dim=0, keepdim=True)).T.contiguous()                     # [k, D] rows, unit norm (as the edit drivers: edit.py:267)
        rows = [(i, a) for i in pcs for a in scales]
        tt = _t_shared(t, 1, "h_traversal")
        out = [eng.forward_shift(x, tt, ctx, key, U, [r[0] for r in rows[i0:i0 + eng.max_batch]], [r[1] for r in rows[i0:i0 + eng.max_batch]], "eps")
               for i0 in range(0, len(rows), eng.max_batch)]
        c, hh, ww = eng.tape.tap_shape[eng.tape.taps["eps"]]
        return torch.cat(out).view(len(pcs), len(scales), c, hh, ww).to(x.dtype)

    # ------------------------------------------------------------------ power iteration
    def _pullback(self, x, t, ctx, op, block_idx, k, chunks, min_iter, max_iter, thr, V0):
        if x.shape[0] != 1:
            raise ValueError("local_encoder_pullback expects a single sample (batch 1), as the reference does")
        if not (1 <= k <= min(self.max_rank, RANK_LIMIT)):
            raise ValueError(f"pca_rank={k} outside [1, {min(self.max_rank, RANK_LIMIT)}] supported by the HIP engine (built for max_rank={self.max_rank} "
                             f"tangents; the library's limit is {RANK_LIMIT})")
        key = self._tap(op, block_idx)
        eng = self.engine
        n_in = eng.n_in
        # One sample on several GPUs (self.k_shard_group set, process group initialised, every rank called with the same inputs): this rank
        # runs the JVP / VJP of its slice of the k directions, one all_gather of W precedes the re-orthonormalisation (dist.py).  W -- and
        # with it V, s and the stop decision -- is identical on every rank.
        import torch.distributed as tdist
        from . import dist as pdist
        shard = self.k_shard_group is not False and tdist.is_available() and tdist.is_initialized() and tdist.get_world_size(self.k_shard_group) > 1
        drawn = V0 is None
        if drawn:
            q, _ = torch.linalg.qr(torch.randn(n_in, k, dtype=torch.float))     # utils.py:750-753 (CPU generator)
            V0 = q.T
        V = V0.reshape(k, n_in).to(device=self.device, dtype=torch.float32).contiguous()
        if shard and drawn:
            # every rank drew from its OWN CPU generator: the ranks must start from one V0, or the row signs orth() aligns to V_prev -- and with
            # them the gathered u_i = +-J v_i -- are rank-specific.  Rank 0 of the group decides.
            Vc = V if tdist.get_backend(self.k_shard_group) == "nccl" else V.cpu()
            tdist.broadcast(Vc, src=tdist.get_global_rank(self.k_shard_group, 0) if self.k_shard_group is not None else 0, group=self.k_shard_group)
            V = Vc.to(self.device)
        time_s = time.time()
        eng.primal(x, _timesteps(t, 1), ctx, key)
        U = s = None
        self.last_history = []                                 # per-iteration ||V_prev - V||_2 (what the reference prints, utils.py:804)
        lo, hi = pdist.k_shard(k, tdist.get_rank(self.k_shard_group), tdist.get_world_size(self.k_shard_group)) if shard else (0, k)
        for i in range(max_iter):
            V_prev = V
            if hi > lo:
                U = torch.cat([eng.jvp(key, vi) for vi in V[lo:hi].chunk(chunks)], dim=0)
                W = torch.cat([eng.vjp(key, ui) for ui in U.chunk(chunks)], dim=0)
            else:
                U, W = V.new_zeros(0, eng.tap_numel(key)), V.new_zeros(0, n_in)
            if shard:
                W = pdist._all_gather_rows(W, k, self.k_shard_group)
            V, s, conv = eng.orth(W, V_prev)
            dist, viol = conv.tolist()                                            # the only host sync per iteration
            self.last_history.append(dist)
            _conv_finite("local_encoder_pullback", i, [[dist, viol]])
            if self.verbose:
                print(f"power method : {i}-th step convergence : ", dist)
            if viol <= thr and i > min_iter:
                if self.verbose:
                    print("reach convergence threshold : ", dist)
                break
        self.last_iters, self.last_dist = i + 1, dist          # introspection for bench.py's time-to-converged-basis leg
        if self.verbose:
            print("power method runtime ==", time.time() - time_s)
        if shard:
            U = pdist._all_gather_rows(U, k, self.k_shard_group)
        dt = x.dtype if x.dtype in (torch.float32, torch.float64) else torch.float32
        return U.T.to(dt), s.to(dt), V.to(dt)

    def local_encoder_pullback_zt(self, sample, timestep, encoder_hidden_states=None, op=None, block_idx=None,
                                  pca_rank=50, chunk_size=25, min_iter=10, max_iter=100, convergence_threshold=1e-3,
                                  V0=None):
        """Reference: src/utils/utils.py:722-816."""
        chunks = max(1, pca_rank // chunk_size)                                   # utils.py:761-764
        return self._pullback(sample, timestep, encoder_hidden_states, op, block_idx, pca_rank, chunks, min_iter, max_iter,
                              convergence_threshold, V0)

    def local_encoder_pullback_xt(self, x, t, op=None, block_idx=None, pca_rank=50, chunk_size=25, min_iter=10,
                                  max_iter=100, convergence_threshold=1e-3, V0=None):
        """Reference: src/utils/utils.py:165-249."""
        chunks = pca_rank // chunk_size if pca_rank % chunk_size == 0 else pca_rank // chunk_size + 1   # utils.py:178
        return self._pullback(x, t, None, op, block_idx, pca_rank, chunks, min_iter, max_iter, convergence_threshold, V0)

    def local_encoder_pullback_batch(self, samples, timesteps, encoder_hidden_states=None, op=None, block_idx=None, pca_rank=50, min_iter=10,
                                     max_iter=100, convergence_threshold=1e-3, V0=None):
        """local_encoder_pullback_zt / _xt of B samples advanced together, each at a timestep of its own: sample b gets what the single-sample
        method returns for (samples[b], timesteps[b], encoder_hidden_states[b]) -- the local tangent spaces of the reference's
        run_sample_encoder_local_tangent_space_zt (src/modules/edit.py:310-383, :1517-1599), whose (sample, t) pairs it visits one call at a time.
        samples [B, ...]; timesteps: one, or B; encoder_hidden_states [1 or B, L, D] (SD); convergence_threshold: a float or B floats; V0: None
        (drawn per sample on the CPU generator, in sample order), [k, N_in] shared or [B, k, N_in].  Returns u [B, N_h, k] (a transposed view,
        columns J V_prev), s [B, k], vT [B, k, N_in] and iters [B] (int64, iterations run for the sample, as last_iters counts them).
        One primal at the B timesteps, then per iteration ONE fused pass of all B * k directions (dpb_pullback_iterate) and one read-back of
        conv [B, 2].  A sample that meets the sign-aligned stop rule (module docstring) at iteration i keeps a snapshot of its (u, s, vT) of
        that iteration; the iterations that go on for the others do not touch it.  Needs B <= max_batch and B * pca_rank <= max_rank."""
        eng = self.engine
        B, k = int(samples.shape[0]), int(pca_rank)
        if not (1 <= B <= eng.max_batch):
            raise ValueError(f"a batch of {B} samples outside [1, max_batch = {eng.max_batch}] of this engine")
        if not (1 <= k <= RANK_LIMIT) or B * k > self.max_rank:
            raise ValueError(f"{B} samples x pca_rank={k} = {B * k} tangents: the engine was built for max_rank={self.max_rank} (max_tangents), and "
                             f"pca_rank must lie in [1, {RANK_LIMIT}]")
        if max_iter < 1:
            raise ValueError(f"max_iter={max_iter} < 1")
        key = self._tap(op, block_idx)
        n_in = eng.n_in
        thr = convergence_threshold
        thr = [float(a) for a in (thr.reshape(-1).tolist() if torch.is_tensor(thr) else thr if isinstance(thr, (list, tuple)) else [thr])]
        if len(thr) not in (1, B):
            raise ValueError(f"convergence_threshold has {len(thr)} entries for a batch of {B}: one or one per sample")
        thr = thr * B if len(thr) == 1 else thr
        if V0 is None:
            V0 = torch.stack([torch.linalg.qr(torch.randn(n_in, k, dtype=torch.float))[0].T for _ in range(B)])   # utils.py:750-753, per sample
        if V0.numel() not in (k * n_in, B * k * n_in):
            raise ValueError(f"V0 has {V0.numel()} elements: [k, N_in] = [{k}, {n_in}] (shared) or [B, k, N_in] with B = {B}")
        V = V0.reshape(-1, n_in).to(device=self.device, dtype=torch.float32)
        V = (V.repeat(B, 1) if V.shape[0] == k and B > 1 else V).contiguous().clone()
        time_s = time.time()
        eng.primal(samples, timesteps, encoder_hidden_states, key)
        n_h = eng.tap_numel(key)
        u_out = torch.empty(B, k, n_h, dtype=torch.float32, device=self.device)
        s_out = torch.empty(B, k, dtype=torch.float32, device=self.device)
        v_out = torch.empty(B, k, n_in, dtype=torch.float32, device=self.device)
        iters = torch.zeros(B, dtype=torch.int64)
        self.last_history = []                                 # per iteration: the B values of ||V_prev - V||_2
        for i in range(max_iter):
            V, U, s, conv = eng.iterate(key, V, 1)
            conv = conv.tolist()                               # the only host sync per iteration
            self.last_history.append([c[0] for c in conv])
            _conv_finite("local_encoder_pullback_batch", i, conv, batch=True)
            if self.verbose:
                print(f"power method : {i}-th step convergence : ", [c[0] for c in conv])
            for b in range(B):
                if iters[b] == 0 and ((conv[b][1] <= thr[b] and i > min_iter) or i == max_iter - 1):
                    iters[b] = i + 1
                    u_out[b], s_out[b], v_out[b] = U.view(B, k, n_h)[b], s.view(B, k)[b], V.view(B, k, n_in)[b]
            if bool((iters > 0).all()):
                break
        self.last_iters = int(iters.max())
        if self.verbose:
            print("power method runtime ==", time.time() - time_s)
        dt = samples.dtype if samples.dtype in (torch.float32, torch.float64) else torch.float32
        return u_out.transpose(1, 2).to(dt), s_out.to(dt), v_out.to(dt), iters

    # ------------------------------------------------------------------ decoder side: h -> eps
    def _decoder_tap(self, op, block_idx):
        key = self._tap(op, block_idx)
        if "eps" not in self.engine.tape.taps:
            raise ValueError("the decoder pullback needs an engine built up to eps: this one was built with upto=... and stops at "
                             f"{[k for k in self.engine.tape.taps][-1]}")
        return key

    def _get_h_to_e(self, sample, timestep, ctx, input_h, op, block_idx, verbose):
        key = self._decoder_tap(op, block_idx)
        b = input_h.shape[0]
        if not (1 <= b <= self.engine.max_batch):
            raise ValueError(f"input_h.size(0) = {b} outside [1, max_batch = {self.engine.max_batch}] of this engine")
        if sample.shape[0] != 1:
            raise ValueError("get_h_to_e expects a single sample (batch 1): its skips are repeated input_h.size(0) times, as the reference does")
        x = sample.expand(b, *sample.shape[1:])
        e = self.engine.forward_from(x, _t_shared(timestep, b, "get_h_to_e"), ctx, key, input_h, "eps")
        if verbose:
            print(f"op : {op}, block_idx : {block_idx}, input_h.shape : {tuple(input_h.shape)}, return eps.shape : {tuple(e.shape)}")
        return e.to(sample.dtype)

    def get_h_to_e(self, *args, **kwargs):
        """eps of the U-Net with the activation at (op, block_idx) replaced by input_h [B, C, H, W] and every skip connection held at its
        value for the single sample given (repeated B times).  SD: get_h_to_e(sample, timestep, encoder_hidden_states, input_h, op,
        block_idx) (utils.py:529-635); uncond: get_h_to_e(x, t, input_h, op, block_idx) (diffusion.py:273-345).  Every tap of the
        engine is accepted (the reference's DDPM code asserts op == 'mid', its SD code takes 'mid' and 'down')."""
        if self.kind == "sd":
            def sd(sample=None, timestep=None, encoder_hidden_states=None, input_h=None, op=None, block_idx=None, verbose=False):
                return self._get_h_to_e(sample, timestep, encoder_hidden_states, input_h, op, block_idx, verbose)
            return sd(*args, **kwargs)

        def ddpm(x=None, t=None, input_h=None, op=None, block_idx=None, verbose=False):
            return self._get_h_to_e(x, t, None, input_h, op, block_idx, verbose)
        return ddpm(*args, **kwargs)

    def _decoder_pullback(self, x, t, ctx, op, block_idx, k, chunks, min_iter, max_iter, thr, V0):
        """Power iteration on J_dec = d eps / d h at one sample: the host-driven loop of _pullback with the passes seeded at the tap.
        Returns (u = V^T [N_h, k] view, s [k], vT = J_dec V_prev [k, N_eps]) in the reference's decoder convention (diffusion.py:626-631)."""
        if x.shape[0] != 1:
            raise ValueError("local_decoder_pullback expects a single sample (batch 1), as the reference does")
        if not (1 <= k <= min(self.max_rank, RANK_LIMIT)):
            raise ValueError(f"pca_rank={k} outside [1, {min(self.max_rank, RANK_LIMIT)}] supported by the HIP engine (built for max_rank={self.max_rank} "
                             f"tangents; the library's limit is {RANK_LIMIT})")
        key = self._decoder_tap(op, block_idx)
        eng = self.engine
        n_h = eng.tap_numel(key)
        if V0 is None:
            q, _ = torch.linalg.qr(torch.randn(n_h, k, dtype=torch.float))        # diffusion.py:585-588 (CPU generator, as _pullback)
            V0 = q.T
        V = V0.reshape(k, n_h).to(device=self.device, dtype=torch.float32).contiguous()
        time_s = time.time()
        eng.primal(x, _timesteps(t, 1), ctx, "eps")
        U = s = None
        self.last_history = []
        for i in range(max_iter):
            V_prev = V
            U = torch.cat([eng.jvp_between(key, "eps", vi) for vi in V.chunk(chunks)], dim=0)
            W = torch.cat([eng.vjp_between(key, "eps", ui) for ui in U.chunk(chunks)], dim=0)
            V, s, conv = eng.orth(W, V_prev)
            dist, viol = conv.tolist()                                            # the only host sync per iteration
            self.last_history.append(dist)
            _conv_finite("local_decoder_pullback", i, [[dist, viol]])
            if self.verbose:
                print(f"power method : {i}-th step convergence : ", dist)
            if thr is not None and viol <= thr and i > min_iter:                # the encoder's sign-aligned allclose rule (module docstring)
                if self.verbose:
                    print("reach convergence threshold : ", dist)
                break
        self.last_iters, self.last_dist = i + 1, dist
        if self.verbose:
            print("power method runtime ==", time.time() - time_s)
        dt = x.dtype if x.dtype in (torch.float32, torch.float64) else torch.float32
        return V.to(dt).T, s.to(dt), U.to(dt)

    def local_decoder_pullback_xt(self, x=None, t=None, op="mid", block_idx=0, pca_rank=50, chunk_size=10, min_iter=10, max_iter=100,
                                  convergence_threshold=1e-3, V0=None):
        """Reference: PullBackDDPM.local_decoder_pullback_xt, src/models/ddpm/diffusion.py:558-632.  Low-rank SVD of J_dec = d eps / d h at
        the tap (op, block_idx) with the skips held at their primal values.  Returns u [N_h, k] (h-space directions, V^T), s = sqrt(singular
        values of J^T J V_prev), vT [k, N_eps] = J_dec V_prev of the last iteration (un-normalised)."""
        chunks = pca_rank // chunk_size if pca_rank % chunk_size == 0 else pca_rank // chunk_size + 1   # diffusion.py:569
        return self._decoder_pullback(x, t, None, op, block_idx, pca_rank, chunks, min_iter, max_iter, convergence_threshold, V0)

    def local_x0_decoder_pullback_xt(self, x=None, t=None, at=None, op="mid", block_idx=0, pca_rank=50, chunk_size=10, num_chunk=None,
                                     min_iter=10, max_iter=100, convergence_threshold=1e-3, V0=None):
        """Reference: PullBackDDPM.local_x0_decoder_pullback_xt, src/models/ddpm/diffusion.py:634-710: the same SVD for
        x0 = (x - sqrt(1 - a_t) eps) / sqrt(a_t).  J_x0 = c J_dec with c = -sqrt(1 - a_t) / sqrt(a_t), so J_x0^T J_x0 = c^2 J_dec^T J_dec
        has the same singular vectors (and the same iterates, stop test included): this is the decoder run with s scaled by |c| and vT by c,
        exactly.  (`num_chunk` is accepted and unused, as in the reference; chunks = pca_rank // chunk_size, at least 1.)"""
        a = at.to(torch.float32) if torch.is_tensor(at) else torch.tensor(float(at), dtype=torch.float32)
        c = float((-(1 - a).sqrt() / a.sqrt()).reshape(-1)[0])
        chunks = max(1, pca_rank // chunk_size)                                   # diffusion.py:664
        u, s, vT = self._decoder_pullback(x, t, None, op, block_idx, pca_rank, chunks, min_iter, max_iter, convergence_threshold, V0)
        return u, s * abs(c), vT * c

    def local_decoder_pullback_zt(self, sample, timestep, encoder_hidden_states=None, op=None, block_idx=None, pca_rank=50, chunk_size=25,
                                  min_iter=10, max_iter=100, convergence_threshold=None, V0=None):
        """Reference: utils.local_decoder_pullback_zt, src/utils/utils.py:818-898 (SD).  Conventions of local_decoder_pullback_xt.
        convergence_threshold=None (the reference's default, on which its own stop test raises: allclose(atol=None) is a TypeError) means
        no early stop: max_iter iterations."""
        chunks = max(1, pca_rank // chunk_size)                                   # utils.py:853, clamped as local_encoder_pullback_zt
        return self._decoder_pullback(sample, timestep, encoder_hidden_states, op, block_idx, pca_rank, chunks, min_iter, max_iter,
                                      convergence_threshold, V0)

    def decoder_pullback_fixed(self, x, t, ctx, op, block_idx, pca_rank, n_iters, V0):
        """pullback_fixed for the decoder: n_iters fused iterations (dpb_pullback_iterate_between), no host synchronisation.
        V0 [b*k, N_h] or [k, N_h] (shared by the b samples); returns (u [N_h, b*k], s, vT [b*k, N_eps], conv [b, 2])."""
        key = self._decoder_tap(op, block_idx)
        eng = self.engine
        eng.primal(x, t, ctx, "eps")                     # (a timestep per sample is honoured)
        b = x.shape[0]
        V = V0.reshape(-1, eng.tap_numel(key)).to(device=self.device, dtype=torch.float32)
        if V.shape[0] == pca_rank and b > 1:
            V = V.repeat(b, 1)
        V, U, s, conv = eng.iterate_between(key, "eps", V.contiguous().clone(), n_iters)
        return V.T, s, U, conv

    def pullback_fixed(self, x, t, ctx, op, block_idx, pca_rank, n_iters, V0):
        """Fixed-iteration variant with no host synchronisation (what bench.py times)."""
        key = self._tap(op, block_idx)
        self.engine.primal(x, t, ctx, key)              # (a timestep per sample is honoured)
        b = x.shape[0]                                  # b samples advance together; V0 is [b*k, N] or [k, N] (shared)
        V = V0.reshape(-1, self.engine.n_in).to(device=self.device, dtype=torch.float32)
        if V.shape[0] == pca_rank and b > 1:
            V = V.repeat(b, 1)
        V, U, s, conv = self.engine.iterate(key, V.contiguous().clone(), n_iters)
        return U.T, s, V, conv


    def pullback_k_sharded(self, x, t, ctx, op, block_idx, pca_rank, n_iters, V0, group=None):
        """ONE sample on several GPUs: the pca_rank directions are dealt to the ranks of `group` (dist.k_sharded_power_iteration); every
        rank calls this with the same x, t, ctx, V0 and gets the same (u [N_h, k], s [k], vT [k, N_in], conv).  For the case the
        sample-sharded path cannot use all GPUs (fewer samples than ranks: the editing CLI's single image)."""
        from . import dist as pdist
        if x.shape[0] != 1:
            raise ValueError("pullback_k_sharded works on a single sample")
        key = self._tap(op, block_idx)
        eng = self.engine
        eng.primal(x, _timesteps(t, 1), ctx, key)
        V = V0.reshape(pca_rank, eng.n_in).to(device=self.device, dtype=torch.float32).contiguous()

        def jtj(Vl):
            U = eng.jvp(key, Vl)
            return U, eng.vjp(key, U)
        U, s, V, conv = pdist.k_sharded_power_iteration(jtj, eng.orth, V, n_iters, group)
        return U.T, s, V, conv

    # ------------------------------------------------------------------ global h-space PCA and h -> x directions
    def global_pca_zt(self, sample=None, timestep=None, encoder_hidden_states=None, op=None, block_idx=None, memory_bound=5, pca_rank=100,
                      pca_device="cpu", x=None, t=None):
        """Reference: utils.global_pca_zt, src/utils/utils.py:978-1027.  h = get_h of every sample (one encoder_hidden_states for all of them, as
        the reference's .repeat), then torch.pca_lowrank(h [N, D], q=pca_rank, center=True, niter=5) -- here dpb_pca_lowrank on the GPU.
        Returns (u [D, q], s [q]) on pca_device in sample.dtype.  R is drawn with torch.randn on pca_device where pca_lowrank draws it, so a seeded
        call with the default pca_device='cpu' uses the reference's own R.  uncond: global_pca_zt(x=..., t=..., op, block_idx).
        Limits: pca_rank <= 128 (RANK_LIMIT), pca_rank <= N - 1, pca_rank <= D."""
        sample = x if sample is None else sample
        timestep = t if timestep is None else timestep
        key = self._tap(op, block_idx)
        eng = self.engine
        n, d, q = sample.shape[0], eng.tap_numel(key), int(pca_rank)
        if eng.lib.dpb_pca_scratch_bytes(q, n, d) == 0:
            raise ValueError(f"pca_rank={q} is not supported for {n} samples of {d} features: 1 <= pca_rank <= min({RANK_LIMIT}, N - 1, D)")
        if memory_bound < 1:
            raise ValueError(f"memory_bound={memory_bound} < 1")
        time_s = time.time()
        tt = _timesteps(timestep, n)                      # one float, or a timestep per sample: sliced with the chunks
        H = torch.empty(n, d, dtype=torch.float32, device=self.device)
        step = min(int(memory_bound), eng.max_batch)     # the reference's chunks hold <= memory_bound samples; the engine's batch bounds them too
        for i0 in range(0, n, step):
            b = min(step, n - i0)
            eng.forward(sample[i0:i0 + b], tt if isinstance(tt, float) else tt[i0:i0 + b], encoder_hidden_states, key, out=H[i0:i0 + b])
        if self.verbose:
            torch.cuda.synchronize(self.device)
            c, hh, ww = eng.tape.tap_shape[eng.tape.taps[key]]
            print("num_pca_samples ==", n)
            print("h sampling t ==", time.time() - time_s)
            print("h shape : ", torch.Size([n, c, hh, ww]))
        time_s = time.time()
        R = torch.randn(min(n, d), q, dtype=torch.float32, device=pca_device)    # torch._lowrank.get_approximate_basis: randn(A.shape[-1], q)
        u, s = pca_lowrank(H, R, q, niter=5)
        s = s.to(device=pca_device, dtype=sample.dtype)
        u = u.T.to(device=pca_device, dtype=sample.dtype)
        if not (torch.isfinite(s).all() and (s > 0).all()):
            raise L.DpbError(f"global_pca_zt: the centred features have rank < pca_rank={q} (singular values {s.tolist()})")
        if self.verbose:
            print("torch.pca_lowrank t ==", time.time() - time_s)
            print(f"eigenvalue spectrum : {s}")
        return u, s

    def inv_jac_zt(self, sample=None, timestep=None, encoder_hidden_states=None, op=None, block_idx=None, u=None, perturb_h=1e-1, x=None, t=None):
        """Reference: utils.inv_jac_zt, src/utils/utils.py:1117-1160: the x-space direction of the h-space direction u at one sample.  The
        reference differentiates ||h + perturb_h u - get_h(x)|| at x, whose gradient is -J^T u / ||u||; so vT = -J^T u / ||J^T u|| (one primal,
        one adjoint pass; perturb_h drops out).  u [D] -> vT [1, N_in].  Extension: u [D, k] (the reference raises NotImplementedError, the
        code after its raise states the result) -> vT [k, N_in], row i from column i, each row normalised; the adjoints run in chunks of max_rank.
        This is one gradient of the objective, not its minimiser: jac_lstsq solves the least-squares problem (with the opposite sign)."""
        sample = x if sample is None else sample
        timestep = t if timestep is None else timestep
        key = self._tap(op, block_idx)
        if sample.shape[0] != 1:
            raise ValueError("sample size should be 1")                         # utils.py:1146
        eng = self.engine
        d = eng.tap_numel(key)
        if u is None or u.numel() % d != 0 or (u.dim() == 1 and u.numel() != d):
            raise ValueError(f"u must be [{d}] or [{d}, k] (features of the tap ({op}, {block_idx}))")
        U = u.reshape(1, d) if u.dim() == 1 else u.reshape(d, -1).T
        U = U.to(device=self.device, dtype=torch.float32).contiguous()
        eng.primal(sample, _t_shared(timestep, 1, "inv_jac"), encoder_hidden_states, key)
        W = torch.cat([eng.vjp(key, ui) for ui in U.split(self.max_rank)], dim=0)
        vT = -W / W.norm(dim=1, keepdim=True)
        return vT.to(sample.dtype)

    # ------------------------------------------------------------------ local h-space PCA: the sampling-based estimate of the local basis
    def local_pca_zt(self, sample=None, timestep=None, encoder_hidden_states=None, op=None, block_idx=None, memory_bound=5, num_pca_samples=50000,
                     pca_rank=RANK_LIMIT, pca_device="cpu", return_x_direction=True, perturb_h=1e-1, x=None, t=None, noise=None, seed=None):
        """Reference: utils.local_pca_zt, src/utils/utils.py:900-975 (uncond: PullBackDDPM.local_pca_xt, src/models/ddpm/diffusion.py:379-436).
        N = num_pca_samples feature rows h_i = get_h(sample + g_i / ||g_i||) of ONE sample (dpb_local_pca_sample: perturbation and forward pass per
        chunk on the device, no host round trip), then torch.pca_lowrank(H [N, D], q=pca_rank, center=True, niter=2) -- dpb_pca_lowrank, with R drawn
        by torch.randn(min(N, D), q) on pca_device where pca_lowrank draws it.  Returns (u [D, q], s [q], vT [q, N_in]) on sample.device in
        sample.dtype (the reference's local variant; the global one returns on pca_device).  vT holds the x-space directions of the columns of u,
        vT_i = -J^T u_i / ||J^T u_i||: the reference differentiates ||h + perturb_h u_i - get_h(x)|| at x, whose gradient for a unit u_i is
        -u_i^T J (perturb_h drops out) -- inv_jac_zt's 2-D path, one primal and the adjoints in chunks of max_rank.
        (Row i belongs to COLUMN i of u, as in PullBackDDPM.inv_jac_xt's rearrange, diffusion.py:360.  utils.local_pca_zt itself adds
        u.view(*original_h.shape), utils.py:960 -- the row-major view of u [D, q] as [q, D] -- so for q > 1 its rows are directions of mixtures of
        all columns; at q = 1 the two agree.  The mixture is not reproduced: it depends on the arbitrary signs of the columns.)
        Extensions: `noise` [N, C, H, W], the unnormalised Gaussian draws g_i (nothing is drawn from any generator before R then); otherwise the
        noise is generated in the kernel from (seed, i) -- Philox4x32-10, include/dpb.h -- with seed=None replaced by ONE torch.randint draw from
        the global CPU generator, so torch.manual_seed governs the call.  The reference's own noise depends on its chunking and on the device
        generator; here sample i's noise never depends on the chunking: memory_bound is validated and otherwise without effect (the chunks are the
        engine's max_batch, which sized the workspace), it never changes the results.  uncond: local_pca_zt(x=..., t=..., op, block_idx).
        Deviations: pca_rank <= 128 (RANK_LIMIT, the default: the reference's defaults of 2000 / 512 exceed the re-orthonormalisation's limit), also
        <= N - 1 and <= D; num_pca_samples % memory_bound != 0 raises ValueError (the DDPM reference asserts, the SD one fails at its view);
        sample.shape[0] != 1 raises ValueError; return_x_direction=False returns vT=None (the reference crashes on None.detach()).
        16-bit engines: the unit-norm perturbation is about 1 / sqrt(N_in) per element -- 0.0078 at the SD latent's 16 384 elements, which is
        the bf16 spacing at 1.0 -- so in a bf16 engine most of the perturbation is lost when x is rounded to the engine's type and the spectrum
        is that of the rounding pattern as much as of J; fp16 keeps three more bits.  The method runs there (finite, descending s); use an fp32
        engine when the basis matters."""
        sample = x if sample is None else sample
        timestep = t if timestep is None else timestep
        key = self._tap(op, block_idx)
        eng = self.engine
        if sample.shape[0] != 1:
            raise ValueError("local_pca expects a single sample (batch 1): every row perturbs the same input")
        n, d, q, mb = int(num_pca_samples), eng.tap_numel(key), int(pca_rank), int(memory_bound)
        if mb < 1:
            raise ValueError(f"memory_bound={memory_bound} < 1")
        if n < 1 or n % mb != 0:
            raise ValueError(f"num_pca_samples={n} must be a positive multiple of memory_bound={mb}")   # diffusion.py:391
        if eng.lib.dpb_pca_scratch_bytes(q, n, d) == 0:
            raise ValueError(f"pca_rank={q} is not supported for {n} samples of {d} features: 1 <= pca_rank <= min({RANK_LIMIT}, N - 1, D)")
        if noise is not None:
            if tuple(noise.shape) != (n, *sample.shape[1:]):
                raise ValueError(f"noise has shape {tuple(noise.shape)}, expected {(n, *sample.shape[1:])} (num_pca_samples unnormalised Gaussian draws)")
        elif seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())      # the global CPU generator: torch.manual_seed governs
        time_s = time.time()
        H = eng.local_pca_sample(sample, _t_shared(timestep, 1, "local_pca"), encoder_hidden_states, key, n, noise=noise, seed=0 if seed is None else int(seed))
        if self.verbose:
            torch.cuda.synchronize(self.device)
            print("h sampling t ==", time.time() - time_s)
        time_s = time.time()
        R = torch.randn(min(n, d), q, dtype=torch.float32, device=pca_device)    # torch._lowrank.get_approximate_basis: randn(A.shape[-1], q)
        ud, sd = pca_lowrank(H, R, q, niter=2)                                    # utils.py:939
        del H
        s = sd.to(device=sample.device, dtype=sample.dtype)
        u = ud.T.to(device=sample.device, dtype=sample.dtype)
        if not (torch.isfinite(s).all() and (s > 0).all()):
            raise L.DpbError(f"local_pca: the centred features have rank < pca_rank={q} (singular values {s.tolist()})")
        if self.verbose:
            print("torch.pca_lowrank t ==", time.time() - time_s)
            print(f"eigenvalue spectrum : {s}")
        vT = None
        if return_x_direction:
            time_s = time.time()
            vT = self.inv_jac_zt(sample, timestep, encoder_hidden_states, op=op, block_idx=block_idx, u=ud.T, perturb_h=perturb_h)
            vT = vT.to(device=sample.device)
            if self.verbose:
                print("torch.jac t ==", time.time() - time_s)
        return u, s, vT

    def local_pca_xt(self, x=None, t=None, op=None, block_idx=None, memory_bound=5, num_pca_samples=50000, pca_rank=RANK_LIMIT, pca_device="cpu",
                     return_x_direction=True, perturb_h=1e-1, noise=None, seed=None):
        """Reference: PullBackDDPM.local_pca_xt, src/models/ddpm/diffusion.py:379-436: local_pca_zt without conditioning (see there)."""
        return self.local_pca_zt(x, t, None, op=op, block_idx=block_idx, memory_bound=memory_bound, num_pca_samples=num_pca_samples, pca_rank=pca_rank,
                                 pca_device=pca_device, return_x_direction=return_x_direction, perturb_h=perturb_h, noise=noise, seed=seed)

    def global_pca_xt(self, x=None, t=None, op=None, block_idx=None, memory_bound=5, pca_rank=100, pca_device="cpu"):
        """Reference: PullBackDDPM.global_pca_xt, src/models/ddpm/diffusion.py:438-482: global_pca_zt without conditioning (its limits; the reference's
        default rank of 512 exceeds them, so the default is global_pca_zt's 100)."""
        return self.global_pca_zt(x, t, None, op=op, block_idx=block_idx, memory_bound=memory_bound, pca_rank=pca_rank, pca_device=pca_device)

    def inv_jac_xt(self, x=None, t=None, op=None, block_idx=None, u=None, perturb_h=1e-1):
        """Reference: PullBackDDPM.inv_jac_xt, src/models/ddpm/diffusion.py:347-377: inv_jac_zt without conditioning; u [D] -> vT [1, N_in], u [D, k]
        -> vT [k, N_in] (the vendored class takes 2-D u).  One gradient of the objective, not its minimiser: jac_lstsq solves the least-squares
        problem (with the opposite sign)."""
        return self.inv_jac_zt(x, t, None, op=op, block_idx=block_idx, u=u, perturb_h=perturb_h)

    # ------------------------------------------------------------------ the parallel-h edit chain
    def inv_jac_chain(self, x=None, t=None, u=None, dirs=None, signs=None, steps=1, step_size=1.0, sega_sigma=None, encoder_hidden_states=None,
                      op=None, block_idx=None, return_vk=False, final_shift=True, check=True):
        """The --edit_xt parallel-h branch of the reference's global-basis edits (src/modules/edit.py:1202-1229, :1470-1497) as one device loop:
        chain b starts at x[b] and takes `steps` steps x <- x + step_size * v with v = inv_jac_xt(x, t, u_b) = -J^T c / ||J^T c|| recomputed at
        every state, c = signs[b] * u[:, dirs[b]] held fixed (dpb_inv_jac_chain: one primal and one adjoint pass per step for all chains together,
        no Python between the steps).  Sign: v is the reference's inv_jac_xt, so a chain with sign +1 moves h AGAINST c -- h_shift is negative at
        first order, about -step_size * ||J^T c|| / ||c|| per step.
        x [n, C, H, W]; t a float or n timesteps; u [D] or [D, k] as inv_jac_* take it (column i is direction i); dirs: n column indices (default:
        0, or 0 .. n-1 when k == n > 1); signs: n floats (default +1); step_size: a float or n; sega_sigma: None or <= 0 off, else v <- where(|v| <
        sega_sigma * std(v), 0, v) at every step (the reference's use_sega_reg).  More chains than the engine's max_batch (or max_rank) run in
        groups; a chain is never split.  Returns a dict of tensors on x.device: states [n, steps + 1, C, H, W] (states[:, 0] = x), norm [n, steps]
        = ||J^T c||, sega_std [n, steps] (0 when off), sega_kept [n, steps] (elements the rule kept; N_in when off), h_shift [n, steps + 1] =
        <h - h0, c> / ||c|| and h_dist [n, steps + 1] = ||h - h0|| at every state (final_shift=False: the last column is NaN and the forward pass
        at the last state is saved), vk [n, steps, N_in] when return_vk.  A chain whose J^T c is zero or not finite at some step has NaN from there
        on: ValueError names the chain and the step, check=False returns the NaNs."""
        key = self._tap(op, block_idx)
        eng = self.engine
        d = eng.tap_numel(key)
        if x is None or x.dim() != 4:
            raise ValueError("x must be [n, C, H, W]")
        n, steps = x.shape[0], int(steps)
        if steps < 1:
            raise ValueError(f"steps={steps} < 1")
        if u is None or u.numel() % d != 0 or (u.dim() == 1 and u.numel() != d):
            raise ValueError(f"u must be [{d}] or [{d}, k] (features of the tap ({op}, {block_idx}))")
        U = u.reshape(1, d) if u.dim() == 1 else u.reshape(d, -1).T
        U = U.to(device=self.device, dtype=torch.float32).contiguous()
        k = U.shape[0]
        if dirs is None:
            dirs = list(range(n)) if k == n and n > 1 else [0] * n
        dirs = [int(a) for a in (dirs.tolist() if torch.is_tensor(dirs) else dirs)]
        signs = [1.0] * n if signs is None else [float(a) for a in (signs.tolist() if torch.is_tensor(signs) else signs)]
        step = step_size.tolist() if torch.is_tensor(step_size) else step_size
        step = [float(a) for a in step] if isinstance(step, (list, tuple)) else [float(step)] * n
        if not (len(dirs) == len(signs) == len(step) == n):
            raise ValueError(f"dirs, signs and step_size need one entry per chain ({n}), got {len(dirs)}, {len(signs)}, {len(step)}")
        if any(a < 0 or a >= k for a in dirs):
            raise ValueError(f"dirs {dirs} outside [0, {k}): u has {k} direction(s)")
        tl = _timesteps(t, n)
        tl = [tl] * n if isinstance(tl, float) else tl
        ctx = encoder_hidden_states
        if ctx is not None and ctx.shape[0] not in (1, n):
            raise ValueError(f"encoder_hidden_states has {ctx.shape[0]} rows for {n} chains: one, or one per chain")
        sigma = 0.0 if sega_sigma is None else float(sega_sigma)
        group = max(1, min(eng.max_batch, eng.max_tangents))
        parts = []
        for b0 in range(0, n, group):
            sl = slice(b0, min(b0 + group, n))
            cg = None if ctx is None else (ctx if ctx.shape[0] == 1 else ctx[sl])
            parts.append(eng.inv_jac_chain(x[sl], tl[sl], cg, key, U, dirs[sl], signs[sl], step[sl], steps, sigma, final_shift, return_vk))
        states = torch.cat([p[0] for p in parts], dim=1).transpose(0, 1).contiguous()
        stats = torch.cat([p[2] for p in parts], dim=1).transpose(0, 1)
        shift = torch.cat([p[3] for p in parts], dim=1).transpose(0, 1)
        out = {"states": states.to(device=x.device, dtype=x.dtype),
               "norm": stats[..., 0].sqrt().to(x.device), "sega_std": stats[..., 1].to(x.device), "sega_kept": stats[..., 2].to(x.device),
               "h_shift": shift[..., 0].to(x.device), "h_dist": shift[..., 1].sqrt().to(x.device)}
        if return_vk:
            out["vk"] = torch.cat([p[1] for p in parts], dim=1).transpose(0, 1).contiguous().to(device=x.device, dtype=x.dtype)
        if check:
            flag = stats[..., 3].cpu()
            if bool((flag != 0).any()):
                b, j = [int(a) for a in (flag != 0).nonzero()[0]]
                raise ValueError(f"inv_jac_chain: chain {b} has no direction at step {j}: ||J^T c||^2 = {float(stats[b, j, 0])} (zero or not finite); "
                                 "check=False returns the NaN states")
        return out

    # ------------------------------------------------------------------ the least-squares inverse of the Jacobian and the newton-h chain
    def _h_directions(self, what, u, key, op, block_idx):
        d = self.engine.tap_numel(key)
        if u is None or u.numel() % d != 0 or (u.dim() == 1 and u.numel() != d):
            raise ValueError(f"{what}: u must be [{d}] or [{d}, k] (features of the tap ({op}, {block_idx}))")
        U = u.reshape(1, d) if u.dim() == 1 else u.reshape(d, -1).T
        return U.to(device=self.device, dtype=torch.float32).contiguous()

    def jac_lstsq(self, x=None, t=None, u=None, damping=0.1, mu=0.0, iters=16, tol=1e-5, encoder_hidden_states=None, op=None, block_idx=None,
                  check=True, sample=None, timestep=None):
        """The x-space step that realises an h-space step: delta = argmin_d ||J d - u||^2 + mu_b ||d||^2 by CGLS from d = 0 (dpb_jac_lstsq: one
        adjoint pass, then `iters` rounds of one tangent and one adjoint pass, no Python between them), where inv_jac_zt / inv_jac_xt give the
        steepest-descent direction -J^T u / ||J^T u|| of the same objective.  With a +u on the right-hand side, h moves ALONG u at first order: the
        opposite sign to inv_jac_* and inv_jac_chain, which keep the reference's.
        One sample x [1, C, H, W] with u [D] or u [D, k] as inv_jac_* take it (column i is right-hand side i), or n samples x [n, C, H, W] with
        u [D, n] (column b belongs to sample b; t a float or n timesteps).  mu_b = mu + damping * ||J^T u_b||^2 / ||u_b||^2: `mu` is the absolute
        Tikhonov term (mu_abs), `damping` the relative one (mu_rel), in units of the squared gain of J along u_b.  For a pure left singular direction
        of J the step shrinks by 1 / (1 + damping); components that J sees `damping` times more weakly (sigma_i^2 = damping * sigma^2) are halved, and
        weaker ones are suppressed in proportion.  tol: a row stops (and freezes) once ||J^T r - mu d|| <= tol * ||J^T u||.
        Returns (delta [k, N_in], info): info["gamma"], ["resid_norm"], ["delta_norm"] are [k, iters + 1] (||J^T r - mu d||^2, ||u - J d||,
        ||d|| after init and after every round), ["iterations"] [k] the rounds a row took, ["converged"] [k] bool (flag 1), ["flag"] [k] and ["mu"]
        [k] = mu_b.  check=True: ValueError names a row with a non-finite input (flag 3); rows that converged (1) or met a zero denominator (2) are
        reported in info, not raised."""
        x = sample if x is None else x
        t = timestep if t is None else t
        key = self._tap(op, block_idx)
        eng = self.engine
        if x is None or x.dim() != 4:
            raise ValueError("jac_lstsq: x must be [n, C, H, W]")
        U = self._h_directions("jac_lstsq", u, key, op, block_idx)
        n, k, iters = x.shape[0], U.shape[0], int(iters)
        if n > 1 and k != n:
            raise ValueError(f"jac_lstsq: {n} samples need u [D, {n}] (one right-hand side per sample), got {k} column(s)")
        if iters < 0:
            raise ValueError(f"jac_lstsq: iters={iters} < 0")
        for name, v in (("damping", damping), ("mu", mu), ("tol", tol)):
            if not (math.isfinite(float(v)) and float(v) >= 0.0):
                raise ValueError(f"jac_lstsq: {name}={v} must be finite and not negative")
        ctx = encoder_hidden_states
        if ctx is not None and ctx.shape[0] not in (1, n):
            raise ValueError(f"encoder_hidden_states has {ctx.shape[0]} rows for {n} samples: one, or one per sample")
        tl = _timesteps(t, n)
        tl = [tl] * n if isinstance(tl, float) else tl
        parts = []
        if n == 1:
            eng.primal(x, tl, ctx, key)
            for Ui in U.split(max(1, eng.max_tangents)):
                parts.append(eng.jac_lstsq(key, Ui, float(mu), float(damping), float(tol), iters))
        else:
            group = max(1, min(eng.max_batch, eng.max_tangents))
            for b0 in range(0, n, group):
                sl = slice(b0, min(b0 + group, n))
                eng.primal(x[sl], tl[sl], None if ctx is None else (ctx if ctx.shape[0] == 1 else ctx[sl]), key)
                parts.append(eng.jac_lstsq(key, U[sl], float(mu), float(damping), float(tol), iters))
        delta = torch.cat([p[0] for p in parts], dim=0)
        hist = torch.cat([p[2] for p in parts], dim=1).transpose(0, 1)           # [k, iters + 1, 4]
        return delta.to(device=x.device, dtype=x.dtype), self._lstsq_info("jac_lstsq", hist, U, float(mu), float(damping), x.device, check)

    @staticmethod
    def _lstsq_info(what, hist, U, mu, damping, device, check):
        """hist [k, iters + 1, 4] fp64 on the engine's device -> the info dict of jac_lstsq"""
        flag = hist[..., 3]
        last = flag[:, -1]
        if check and bool((last == 3).any()):
            b = int((last == 3).nonzero()[0])
            j = int((flag[b] == 3).nonzero()[0])
            raise ValueError(f"{what}: row {b} met a non-finite input at " + ("the start" if j == 0 else f"iteration {j}") +
                             "; check=False returns the NaN row")
        live = (flag == 0).sum(dim=1)                                             # rows of hist written while the row was live
        gamma0 = hist[:, 0, 0]
        info = {"gamma": hist[..., 0], "resid_norm": hist[..., 1].sqrt(), "delta_norm": hist[..., 2].sqrt(),
                "iterations": torch.clamp(live, max=hist.shape[1] - 1).to(torch.int64), "converged": last == 1, "flag": last.to(torch.int64)}
        cc = (U.double() ** 2).sum(dim=1)
        info["mu"] = mu + damping * torch.where(cc > 0, gamma0 / cc, torch.zeros_like(cc))      # mu_b as the solver forms it (0 / 0: mu alone)
        return {k_: v.to(device) for k_, v in info.items()}

    def newton_h_chain(self, x=None, t=None, u=None, dirs=None, signs=None, scale=1.0, steps=4, iters=8, damping=0.1, mu=0.0, tol=1e-5, radius=None,
                       encoder_hidden_states=None, op=None, block_idx=None, final_shift=True, check=True):
        """A damped Gauss-Newton chain towards an h-space target, as one device loop (dpb_newton_h_chain): chain b starts at x[b] and aims at
        h0_b + scale_b * c_b, c_b = signs[b] * u[:, dirs[b]].  Outer step j of `steps`: one primal pass at the state, the residual
        res = h0 + ((j + 1) / steps) * scale_b * c_b - h, the inner solve of jac_lstsq on it (`iters` CGLS rounds with `damping`, `mu`, `tol`), and
        x <- x + kappa * delta with kappa = min(1, radius / ||delta||) (radius None or 0: no clamp).  Where inv_jac_chain follows the steepest-descent
        direction -J^T c / ||J^T c|| and drifts towards what J amplifies most, this chain takes the least-squares step, so its off-axis distance h_off
        stays smaller at the same shift.  Sign: a chain with sign +1 moves h ALONG c (h_shift > 0) -- the opposite of inv_jac_chain, which keeps the
        reference's sign.  `scale` is in h units (the shift asked for), a float or n floats.
        x [n, C, H, W]; t a float or n timesteps; u, dirs, signs as inv_jac_chain takes them.  More chains than min(max_batch, max_rank) run in
        groups; a chain is never split.  Returns a dict of tensors on x.device: states [n, steps + 1, C, H, W]; h_shift, h_dist [n, steps + 1] as
        inv_jac_chain's (final_shift=False: the last column is NaN); h_off = sqrt(max(0, h_dist^2 - h_shift^2)); resid_norm [n, steps] = ||res|| at
        the start of each step; delta_norm [n, steps] = ||delta|| before the clamp; clip [n, steps] = kappa; inner_iterations [n, steps]; gamma
        [n, steps, iters + 1]; flag [n, steps].  check=True: ValueError names a chain and step with a non-finite input (flag 3)."""
        key = self._tap(op, block_idx)
        eng = self.engine
        if x is None or x.dim() != 4:
            raise ValueError("newton_h_chain: x must be [n, C, H, W]")
        n, steps, iters = x.shape[0], int(steps), int(iters)
        if steps < 1:
            raise ValueError(f"newton_h_chain: steps={steps} < 1")
        if iters < 0:
            raise ValueError(f"newton_h_chain: iters={iters} < 0")
        U = self._h_directions("newton_h_chain", u, key, op, block_idx)
        k = U.shape[0]
        if dirs is None:
            dirs = list(range(n)) if k == n and n > 1 else [0] * n
        dirs = [int(a) for a in (dirs.tolist() if torch.is_tensor(dirs) else dirs)]
        signs = [1.0] * n if signs is None else [float(a) for a in (signs.tolist() if torch.is_tensor(signs) else signs)]
        sc = scale.tolist() if torch.is_tensor(scale) else scale
        sc = [float(a) for a in sc] if isinstance(sc, (list, tuple)) else [float(sc)] * n
        if not (len(dirs) == len(signs) == len(sc) == n):
            raise ValueError(f"newton_h_chain: dirs, signs and scale need one entry per chain ({n}), got {len(dirs)}, {len(signs)}, {len(sc)}")
        if any(a < 0 or a >= k for a in dirs):
            raise ValueError(f"newton_h_chain: dirs {dirs} outside [0, {k}): u has {k} direction(s)")
        radius = 0.0 if radius is None else float(radius)
        for name, v in (("damping", damping), ("mu", mu), ("tol", tol), ("radius", radius)):
            if not (math.isfinite(float(v)) and float(v) >= 0.0):
                raise ValueError(f"newton_h_chain: {name}={v} must be finite and not negative")
        tl = _timesteps(t, n)
        tl = [tl] * n if isinstance(tl, float) else tl
        ctx = encoder_hidden_states
        if ctx is not None and ctx.shape[0] not in (1, n):
            raise ValueError(f"encoder_hidden_states has {ctx.shape[0]} rows for {n} chains: one, or one per chain")
        group = max(1, min(eng.max_batch, eng.max_tangents))
        parts = []
        for b0 in range(0, n, group):
            sl = slice(b0, min(b0 + group, n))
            cg = None if ctx is None else (ctx if ctx.shape[0] == 1 else ctx[sl])
            parts.append(eng.newton_h_chain(x[sl], tl[sl], cg, key, U, dirs[sl], signs[sl], sc[sl], steps, iters, float(mu), float(damping), float(tol),
                                            radius, final_shift))
        states = torch.cat([p[0] for p in parts], dim=1).transpose(0, 1).contiguous()
        hist = torch.cat([p[1] for p in parts], dim=2).permute(2, 0, 1, 3)        # [n, steps, iters + 1, 4]
        stats = torch.cat([p[2] for p in parts], dim=1).transpose(0, 1)           # [n, steps, 4]
        shift = torch.cat([p[3] for p in parts], dim=1).transpose(0, 1)
        if check and bool((stats[..., 3] == 3).any()):
            b, j = [int(a) for a in (stats[..., 3] == 3).nonzero()[0]]
            raise ValueError(f"newton_h_chain: chain {b} met a non-finite value in outer step {j}; check=False returns the NaN states")
        a, q = shift[..., 0], shift[..., 1]
        live = (hist[..., 3] == 0).sum(dim=2)
        out = {"states": states.to(device=x.device, dtype=x.dtype), "h_shift": a, "h_dist": q.sqrt(), "h_off": torch.clamp(q - a * a, min=0.0).sqrt(),
               "resid_norm": stats[..., 0].sqrt(), "delta_norm": stats[..., 1].sqrt(), "clip": stats[..., 2],
               "inner_iterations": torch.clamp(live, max=iters).to(torch.int64), "gamma": hist[..., 0], "flag": stats[..., 3].to(torch.int64)}
        return {k_: v.to(x.device) for k_, v in out.items()}


    # ------------------------------------------------------------------ the h-space guidance edit
    def h_space_guidance(self, x=None, timesteps=None, alphas=None, alphas_next=None, u=None, dirs=None, scales=None, mode="asyrp",
                         encoder_hidden_states=None, op=None, block_idx=None, check=True):
        """The edit_ht == 'h_space_guidance' branch of the reference's global-basis edits (src/modules/edit.py:1232-1245, :1500-1513, which call a
        method the reference never defines) as Kwon et al. state it (Asyrp), one device loop (dpb_hguide_chain): chain b starts at x[b] and runs
        the S DDIM steps (timesteps[j], alphas[j]) -> alphas_next[j]; at every step the net runs plain (e) and with scales[b] * u[:, dirs[b]] /
        ||u[:, dirs[b]]|| added at the tap (op, block_idx) (e_s), and with d = e_s - e the step is
            P = (x - (e + gP d) sqrt(1 - a)) / sqrt(a),   x' = sqrt(a_next) P + sqrt(1 - a_next) (e + gD d)                      (eta = 0).
        mode: "asyrp" (gP, gD) = (1, 0), the asymmetric reverse process; "symmetric" (1, 1), the plain DDIM step of the shifted net; or a pair of
        finite floats.  x [n, C, H, W]; timesteps / alphas / alphas_next: S floats each, shared by the chains (scheduler.ddim_triples gives them);
        u [D] or [D, k] columns as the pullbacks and PCAs return them, normalised here as in h_traversal; dirs: n column indices (default: 0, or
        0 .. n-1 when k == n > 1); scales: a float or n.  A step runs 2n rows: more chains than max_batch // 2 run in groups.  Returns a dict of
        tensors on x.device: states [n, S + 1, C, H, W] (states[:, 0] = x), delta_norm [n, S] = ||d||, dx_norm [n, S] = |-sqrt(a_next)
        sqrt(1 - a) / sqrt(a) gP + sqrt(1 - a_next) gD| ||d||, the distance from the plain DDIM step.  A chain that meets a non-finite value has NaN
        from there on: ValueError names the chain and the step, check=False returns the NaNs.  Classifier-free guidance is not part of the chain:
        SD takes the encoder_hidden_states rows it is given (one, or one per chain)."""
        key = self._decoder_tap(op, block_idx)
        eng = self.engine
        d = eng.tap_numel(key)
        if x is None or x.dim() != 4:
            raise ValueError("x must be [n, C, H, W]")
        n = x.shape[0]
        if isinstance(mode, str):
            if mode not in ("asyrp", "symmetric"):
                raise ValueError(f"mode {mode!r}: 'asyrp', 'symmetric' or a pair (gP, gD)")
            gP, gD = (1.0, 0.0) if mode == "asyrp" else (1.0, 1.0)
        else:
            gP, gD = (float(a) for a in mode)
        if not (math.isfinite(gP) and math.isfinite(gD)):
            raise ValueError(f"mode ({gP}, {gD}) is not finite")
        as_list = lambda a: [float(v) for v in (a.reshape(-1).tolist() if torch.is_tensor(a) else a)]
        tl, al, an = as_list(timesteps), as_list(alphas), as_list(alphas_next)
        S = len(tl)
        if S < 1 or len(al) != S or len(an) != S:
            raise ValueError(f"timesteps, alphas and alphas_next need the same number (>= 1) of entries, got {S}, {len(al)}, {len(an)}")
        if u is None or u.numel() == 0 or u.numel() % d != 0 or (u.dim() == 1 and u.numel() != d) or (u.dim() == 2 and u.shape[0] != d) or u.dim() > 2:
            raise ValueError(f"u must be [{d}] or [{d}, k] (columns: directions at the tap ({op}, {block_idx}))")
        U = u.detach().reshape(d, -1).to(device=self.device, dtype=torch.float32)
        U = (U / U.norm(dim=0, keepdim=True)).T.contiguous()                     # [k, D] rows, unit norm (as h_traversal)
        k = U.shape[0]
        if dirs is None:
            dirs = list(range(n)) if k == n and n > 1 else [0] * n
        dirs = [int(a) for a in (dirs.tolist() if torch.is_tensor(dirs) else dirs)]
        sc = scales.tolist() if torch.is_tensor(scales) else scales
        sc = [float(a) for a in sc] if isinstance(sc, (list, tuple)) else [float(sc)] * n
        if len(dirs) != n or len(sc) != n:
            raise ValueError(f"dirs and scales need one entry per chain ({n}), got {len(dirs)}, {len(sc)}")
        if any(a < 0 or a >= k for a in dirs):
            raise ValueError(f"dirs {dirs} outside [0, {k}): u has {k} direction(s)")
        ctx = encoder_hidden_states
        if ctx is not None and ctx.shape[0] not in (1, n):
            raise ValueError(f"encoder_hidden_states has {ctx.shape[0]} rows for {n} chains: one, or one per chain")
        group = eng.max_batch // 2
        if group < 1:
            raise ValueError(f"h_space_guidance runs a plain and a shifted row per chain: the engine needs max_batch >= 2, has {eng.max_batch}")
        parts = []
        for b0 in range(0, n, group):
            sl = slice(b0, min(b0 + group, n))
            cg = None if ctx is None else (ctx if ctx.shape[0] == 1 else ctx[sl])
            parts.append(eng.hguide_chain(x[sl], tl, al, an, cg, key, U, dirs[sl], sc[sl], gP, gD))
        states = torch.cat([p[0] for p in parts], dim=1).transpose(0, 1).contiguous()
        delta = torch.cat([p[1] for p in parts], dim=1).transpose(0, 1)          # [n, S, 2] fp64
        a_t, a_n = torch.tensor(al, dtype=torch.float64), torch.tensor(an, dtype=torch.float64)
        coef = (-a_n.sqrt() * (1 - a_t).sqrt() / a_t.sqrt() * gP + (1 - a_n).sqrt() * gD).abs()
        dn = delta[..., 0].sqrt().to(x.device)
        out = {"states": states.to(device=x.device, dtype=x.dtype), "delta_norm": dn, "dx_norm": dn * coef.to(x.device)}
        if check:
            flag = delta[..., 1].cpu()
            if bool((flag != 0).any()):
                b, j = [int(a) for a in (flag != 0).nonzero()[0]]
                raise ValueError(f"h_space_guidance: chain {b} holds a non-finite value at step {j}; check=False returns the NaN states")
        return out

    # ------------------------------------------------------------------ pullback geodesics between two latents
    def _curve_args(self, what, curve, t, op, block_idx, encoder_hidden_states, lam):
        """the checks pullback_geodesic and curve_energy share, made before anything runs: (tap key, m, t, ctx, lam)"""
        key = self._tap(op, block_idx)
        eng = self.engine
        if curve is None or curve.dim() != 4 or tuple(curve.shape[1:]) != tuple(self.in_shape):
            raise ValueError(f"{what}: the curve must be [m + 2, {', '.join(str(a) for a in self.in_shape)}]")
        m = curve.shape[0] - 2
        if m < 1:
            raise ValueError(f"{what}: n_points={m} < 1: a curve has two end points and at least one point between them")
        if m + 2 > eng.max_batch:
            raise ValueError(f"{what}: a curve of {m + 2} points is longer than the engine's max_batch={eng.max_batch}: its points are coupled and "
                             "run as one batch (a longer curve is not split)")
        if m > eng.max_tangents:
            raise ValueError(f"{what}: n_points={m} above the engine's max_rank={eng.max_tangents}: the adjoint pass carries one cotangent per point")
        lam = float(lam)
        if not math.isfinite(lam) or lam < 0:
            raise ValueError(f"{what}: lam={lam} must be finite and >= 0")
        ctx = encoder_hidden_states
        if ctx is not None and ctx.shape[0] not in (1, m + 2):
            raise ValueError(f"{what}: encoder_hidden_states has {ctx.shape[0]} rows for a curve of {m + 2} points: one, or one per point")
        if ctx is not None and ctx.shape[0] == 1:
            ctx = ctx.expand(m + 2, *ctx.shape[1:])
        return key, m, _t_shared(t, m + 2, what), ctx, lam

    def curve_energy(self, curve=None, t=None, op=None, block_idx=None, encoder_hidden_states=None, lam=0.0):
        """The ruler of pullback_geodesic, without optimisation: curve [m + 2, C, H, W] at ONE timestep t -> a dict with seg_h, seg_x [m + 1] fp64
        (||h_{i+1} - h_i||^2 at the tap (op, block_idx) and ||P_{i+1} - P_i||^2), energy_h = 1/2 sum seg_h, energy_x = 1/2 sum seg_x, energy =
        energy_h + lam energy_x, length_h = sum sqrt(seg_h), length_x, and uniformity = length_h^2 / ((m + 1) sum seg_h) (1 when the h-segments are
        equal: a discrete geodesic has constant speed).  No chain: get_h of the two end points as one batch and of the m interior points as another
        -- the two batches dpb_geodesic_chain runs, so the figures of a chain's last row are these bit for bit -- then dpb_geodesic_cotangents on
        the activations and on the curve itself.  Lets lerp, slerp and the geodesic be measured alike.  A curve longer than max_batch is refused."""
        from .engine import geodesic_cotangents
        key, m, t, ctx, lam = self._curve_args("curve_energy", curve, t, op, block_idx, encoder_hidden_states, lam)
        eng = self.engine
        P = curve.detach().to(device=self.device, dtype=torch.float32).contiguous()
        ends = torch.stack([P[0], P[m + 1]])
        h = torch.empty(m + 2, eng.tap_numel(key), dtype=torch.float32, device=self.device)
        he = eng.forward(ends, t, None if ctx is None else torch.stack([ctx[0], ctx[m + 1]]), key).flatten(1)
        h[0], h[m + 1] = he[0], he[1]
        eng.forward(P[1:m + 1], t, None if ctx is None else ctx[1:m + 1], key, out=h[1:m + 1])
        seg_h = geodesic_cotangents(h, return_csq=False)[1]
        seg_x = geodesic_cotangents(P.flatten(1), return_csq=False)[1]
        return _curve_stats(seg_h.cpu(), seg_x.cpu(), lam)

    def pullback_geodesic(self, x_a=None, x_b=None, t=None, n_points=8, op=None, block_idx=None, encoder_hidden_states=None, init="slerp", lam=0.0,
                          step_size=None, max_iter=200, tol=1e-4, check_every=4, max_halvings=8, check=True):
        """The shortest path from x_a to x_b [1, C, H, W] or [C, H, W] at ONE timestep t under the pullback metric G = J^T J of h = get_h(x, t) at
        the tap (op, block_idx), as a discrete curve of m = n_points interior points between the fixed ends: gradient descent on
            E = 1/2 sum_i ||h_{i+1} - h_i||^2 + 1/2 lam sum_i ||P_{i+1} - P_i||^2,    g_i = J(P_i)^T (2 h_i - h_{i-1} - h_{i+1}) + lam (2 P_i - P_{i-1} - P_{i+1}),
        by Jacobi steps P_i <- P_i - eta g_i on the device (dpb_geodesic_chain: per iteration one primal and one adjoint pass of the m points, no
        Python between the iterations of a block).  lam = 0 (default) is well posed: g_i lies in the row space of J, what J does not see of the
        start curve is kept.  init: "slerp", "linear", or a tensor [m + 2, C, H, W] whose end rows equal x_a and x_b.  encoder_hidden_states (SD):
        one row for the whole curve, or m + 2.
        The driver (host): blocks of check_every iterations at one eta, each read back once.  A block whose end energy is not finite or above its
        start energy is discarded and eta <- eta / 2 -- after max_halvings such halvings in a row the descent stops, converged=False; an accepted
        block ends the descent with converged=True when E_start - E_end <= tol E_start.  max_iter bounds the iterations run, discarded ones
        included.  step_size=None: eta_0 = 1/4 sum_i ||c_i||^2 / sum_i ||g_i||^2 from a one-iteration probe block with eta = 0 (the csq output of
        dpb_geodesic_cotangents and the ||g||^2 of dpb_geodesic_update).
        Returns (curve [m + 2, C, H, W] on x_a.device, info): info holds energy (a list: E at every accepted block boundary, the start included),
        energy_h, energy_x, length_h, length_x, uniformity, seg_h, seg_x (the final curve's, as curve_energy gives them), grad_norm [m] (||g_i|| at
        the last iteration taken), step_size (the final eta), iterations (accepted), attempted (all), halvings, decisions (a bool per block),
        converged, monotone (the energies of `energy` never rise: what the block rule guarantees), rises (the iterations INSIDE accepted blocks at
        which E rose -- a Jacobi chain at one eta may rise and come back within a block; check_every=1 sees every one) and start = {energy, length_h,
        uniformity} of the initial curve.
        A point that meets a non-finite value at the first iteration of a block (the curve itself, or its adjoint): ValueError names the point and
        the iteration; check=False returns the curve after that iteration, with NaN in the rows it reached -- the point's own and its two
        neighbours', whose cotangents read its activation -- and every other row as the clean step leaves it.  A curve longer than max_batch is
        refused."""
        if x_a is None or x_b is None:
            raise ValueError("pullback_geodesic: x_a and x_b are needed")
        shape = tuple(self.in_shape)
        xa, xb = (x.detach().unsqueeze(0) if x.dim() == 3 else x.detach() for x in (x_a, x_b))
        if tuple(xa.shape) != (1, *shape) or tuple(xb.shape) != (1, *shape):
            raise ValueError(f"pullback_geodesic: x_a and x_b must be one sample of shape {shape} each, got {tuple(x_a.shape)} and {tuple(x_b.shape)}")
        m, max_iter, check_every, max_halvings = int(n_points), int(max_iter), int(check_every), int(max_halvings)
        if m < 1:
            raise ValueError(f"pullback_geodesic: n_points={m} < 1")
        if max_iter < 1 or check_every < 1 or max_halvings < 0:
            raise ValueError(f"pullback_geodesic: max_iter={max_iter} and check_every={check_every} must be >= 1, max_halvings={max_halvings} >= 0")
        tol = float(tol)
        if not math.isfinite(tol) or tol < 0:
            raise ValueError(f"pullback_geodesic: tol={tol} must be finite and >= 0")
        if step_size is not None and not (math.isfinite(float(step_size)) and float(step_size) > 0):
            raise ValueError(f"pullback_geodesic: step_size={step_size} must be finite and > 0 (None: the step rule)")
        P0 = geodesic_init(xa[0], xb[0], m, init)
        key, m, t, ctx, lam = self._curve_args("pullback_geodesic", P0, t, op, block_idx, encoder_hidden_states, lam)
        eng = self.engine

        def block(P, eta, iters, final=True):
            curves, seg_h, seg_x, stats, csq = eng.geodesic_chain(P, t, ctx, key, eta, lam, iters, final)
            return curves, seg_h.cpu(), seg_x.cpu(), stats.cpu(), csq.cpu()
        curve, info = geodesic_descent(block, P0.to(self.device), lam, None if step_size is None else float(step_size), max_iter, tol, check_every,
                                       max_halvings, check)
        return curve.to(device=x_a.device, dtype=x_a.dtype), info


def geodesic_init(xa: torch.Tensor, xb: torch.Tensor, m: int, init="slerp") -> torch.Tensor:
    """the start curve [m + 2, C, H, W] fp32 between xa and xb [C, H, W]: "linear" x_a + s (x_b - x_a), "slerp" sin((1 - s) w) / sin w x_a + sin(s w)
    / sin w x_b with w the angle between the two (linear when sin w < 1e-6), s = i / (m + 1), formed in float64; or a tensor of that shape whose end
    rows equal xa and xb.  The end rows are xa and xb themselves, bit for bit."""
    a, b = xa.detach().to(torch.float32), xb.detach().to(torch.float32)
    if torch.is_tensor(init):
        P = init.detach().to(device=a.device, dtype=torch.float32)
        if tuple(P.shape) != (m + 2, *a.shape):
            raise ValueError(f"pullback_geodesic: init has shape {tuple(P.shape)}, expected {(m + 2, *a.shape)} (n_points + 2 rows)")
        if not (torch.equal(P[0], a) and torch.equal(P[-1], b)):
            raise ValueError("pullback_geodesic: the end rows of init must equal x_a and x_b")
        return P.contiguous()
    if init not in ("slerp", "linear"):
        raise ValueError(f"pullback_geodesic: init {init!r}: 'slerp', 'linear' or a tensor [n_points + 2, C, H, W]")
    a64, b64 = a.double().cpu(), b.double().cpu()
    s = (torch.arange(m + 2, dtype=torch.float64) / (m + 1)).view(-1, *([1] * a.dim()))
    wa, wb = 1 - s, s
    if init == "slerp":
        c = float((a64 * b64).sum() / (a64.norm() * b64.norm()).clamp_min(1e-300))
        w = math.acos(max(-1.0, min(1.0, c)))
        if math.sin(w) >= 1e-6:
            wa, wb = torch.sin((1 - s) * w) / math.sin(w), torch.sin(s * w) / math.sin(w)
    P = (wa * a64 + wb * b64).to(torch.float32).to(a.device)
    P[0], P[-1] = a, b
    return P.contiguous()


def _curve_stats(seg_h: torch.Tensor, seg_x: torch.Tensor, lam: float) -> dict:
    """the statistics of one curve from its segment sums (fp64, on the host)"""
    seg_h, seg_x = seg_h.double(), seg_x.double()
    eh, ex = 0.5 * float(seg_h.sum()), 0.5 * float(seg_x.sum())
    lh = float(seg_h.sqrt().sum())
    return {"energy": eh + lam * ex, "energy_h": eh, "energy_x": ex, "length_h": lh, "length_x": float(seg_x.sqrt().sum()),
            "uniformity": lh * lh / (seg_h.numel() * float(seg_h.sum())) if float(seg_h.sum()) > 0 else float("nan"), "seg_h": seg_h, "seg_x": seg_x}


def geodesic_descent(block, P0, lam, step_size, max_iter, tol, check_every, max_halvings, check=True):
    """The host driver of pullback_geodesic.  block(P, eta, iters, final) -> (curves [iters + 1, m + 2, ...] on the device, and on the host seg_h,
    seg_x [iters + 1, m + 1], stats [iters, m, 4], csq [iters, m]) is one dpb_geodesic_chain call.  Returns (curve, info); the rules are those of
    PullbackUNet.pullback_geodesic."""
    E = lambda sh, sx: 0.5 * float(sh.double().sum()) + lam * 0.5 * float(sx.double().sum())

    def flagged(stats, j):
        bad = (stats[j, :, 3] != 0).nonzero()
        return None if bad.numel() == 0 else int(bad[0]) + 1

    curve, attempted, row, energy, last = P0, 0, 0, [], None       # last: (seg_h, seg_x, stats row) of the curve held
    info = {"halvings": 0, "decisions": [], "converged": False, "rises": 0, "iterations": 0}
    if step_size is None:                            # the probe: one iteration at eta = 0 moves nothing and yields ||c||^2 and ||g||^2
        _, _, _, st, csq = block(curve, 0.0, 1, False)
        c2, g2 = float(csq[0].double().sum()), float(st[0, :, 1].double().sum())
        # (a stationary curve, g = 0, or a non-finite one: any eta -- the first block accepts the one and reports the other)
        eta = 0.25 * c2 / g2 if g2 > 0 and math.isfinite(c2 / g2) and c2 > 0 else 1.0
    else:
        eta = step_size
    while attempted < max_iter:
        n = min(check_every, max_iter - attempted)
        curves, sh, sx, st, _ = block(curve, eta, n, True)
        attempted += n
        if not energy:
            energy.append(E(sh[0], sx[0]))
            info["start"] = {k: _curve_stats(sh[0], sx[0], lam)[k] for k in ("energy", "length_h", "uniformity")}
            last = (sh[0], sx[0], st[0])
        bad = flagged(st, 0)
        if bad is not None:
            if check:
                # a point that is not finite itself flags its two neighbours as well (they read its activation): name the point, not the neighbours
                own = (~torch.isfinite(curves[0]).flatten(1).all(1)).nonzero().flatten().tolist()
                bad = own[0] if own else bad
                raise ValueError(f"pullback_geodesic: point {bad} of the curve " + ("is not finite" if own else "meets a non-finite activation or "
                                 f"adjoint J^T c") + f" at iteration {info['iterations']}; check=False returns the NaN rows")
            curve, last = curves[1], (sh[1], sx[1], st[0])
            break
        e0, e1 = E(sh[0], sx[0]), E(sh[n], sx[n])
        ok = math.isfinite(e1) and e1 <= e0
        info["decisions"].append(ok)
        if not ok:
            eta, row = eta / 2, row + 1
            info["halvings"] += 1
            if row >= max_halvings:
                break
            continue
        row = 0
        es = [E(sh[j], sx[j]) for j in range(n + 1)]
        info["rises"] += sum(es[j + 1] > es[j] for j in range(n))
        curve, last = curves[n], (sh[n], sx[n], st[n - 1])
        info["iterations"] += n
        energy.append(e1)
        if e0 - e1 <= tol * e0:
            info["converged"] = True
            break
    info.update(_curve_stats(last[0], last[1], lam))
    info.update(energy=energy, monotone=all(b <= a for a, b in zip(energy, energy[1:])), grad_norm=last[2][:, 1].double().sqrt(), step_size=eta,
                attempted=attempted)
    return curve, info


def bind(unet, kind: str, cfg, dtype=torch.float32, device="cuda:0", **kw) -> PullbackUNet:
    """Attach the HIP-backed methods onto an existing U-Net module, like the reference's
    ``types.MethodType`` injection (utils.py:103-104, :326-337).  ``unet.state_dict()`` uses diffusers' keys: ``UNet2DConditionModel`` for "sd"
    (consumed as is by tape.build_sd), ``UNet2DModel`` for "ddpm" (renamed by weights.ddpm_hf_to_vendored_names; the vendored
    naming of src/models/ddpm/diffusion.py is accepted unchanged), guided-diffusion ``UNetModel`` for "adm" (consumed as is by tape.build_adm)."""
    sd = {k: v.detach().cpu() for k, v in unet.state_dict().items()}
    if kind == "ddpm":                    # diffusers UNet2DModel keys (the reference's live path, utils.py:101-104) -> builder names
        from .weights import ddpm_hf_to_vendored_names
        sd = ddpm_hf_to_vendored_names(sd, cfg)
    impl = PullbackUNet(kind, cfg, sd, dtype, device, **kw)
    unet._dpb = impl
    unet.get_h = types.MethodType(lambda self, *a, **k: self._dpb.get_h(*a, **k), unet)
    unet.get_h_to_e = types.MethodType(lambda self, *a, **k: self._dpb.get_h_to_e(*a, **k), unet)
    unet.local_encoder_pullback_batch = types.MethodType(lambda self, *a, **k: self._dpb.local_encoder_pullback_batch(*a, **k), unet)
    unet.inv_jac_chain = types.MethodType(lambda self, *a, **k: self._dpb.inv_jac_chain(*a, **k), unet)
    unet.jac_lstsq = types.MethodType(lambda self, *a, **k: self._dpb.jac_lstsq(*a, **k), unet)
    unet.newton_h_chain = types.MethodType(lambda self, *a, **k: self._dpb.newton_h_chain(*a, **k), unet)
    unet.h_space_guidance = types.MethodType(lambda self, *a, **k: self._dpb.h_space_guidance(*a, **k), unet)
    unet.pullback_geodesic = types.MethodType(lambda self, *a, **k: self._dpb.pullback_geodesic(*a, **k), unet)
    unet.curve_energy = types.MethodType(lambda self, *a, **k: self._dpb.curve_energy(*a, **k), unet)
    if kind == "sd":
        unet.local_encoder_pullback_zt = types.MethodType(lambda self, *a, **k: self._dpb.local_encoder_pullback_zt(*a, **k), unet)
        unet.local_decoder_pullback_zt = types.MethodType(lambda self, *a, **k: self._dpb.local_decoder_pullback_zt(*a, **k), unet)
        unet.global_pca_zt = types.MethodType(lambda self, *a, **k: self._dpb.global_pca_zt(*a, **k), unet)
        unet.inv_jac_zt = types.MethodType(lambda self, *a, **k: self._dpb.inv_jac_zt(*a, **k), unet)
        unet.forward_dh = types.MethodType(lambda self, *a, **k: self._dpb.forward_dh(*a, **k), unet)
        unet.local_pca_zt = types.MethodType(lambda self, *a, **k: self._dpb.local_pca_zt(*a, **k), unet)
    else:
        unet.local_encoder_pullback_xt = types.MethodType(lambda self, *a, **k: self._dpb.local_encoder_pullback_xt(*a, **k), unet)
        unet.local_decoder_pullback_xt = types.MethodType(lambda self, *a, **k: self._dpb.local_decoder_pullback_xt(*a, **k), unet)
        unet.local_x0_decoder_pullback_xt = types.MethodType(lambda self, *a, **k: self._dpb.local_x0_decoder_pullback_xt(*a, **k), unet)
        unet.local_pca_xt = types.MethodType(lambda self, *a, **k: self._dpb.local_pca_xt(*a, **k), unet)
        unet.global_pca_xt = types.MethodType(lambda self, *a, **k: self._dpb.global_pca_xt(*a, **k), unet)
        unet.inv_jac_xt = types.MethodType(lambda self, *a, **k: self._dpb.inv_jac_xt(*a, **k), unet)
    return impl
