"""Runtime wrapper around one libdpb engine (one per GPU per process).

PyTorch is used for device memory (workspace / IO tensors) and the current HIP stream only;
all arithmetic happens in the HIP kernels behind the C ABI (include/dpb.h).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import lib as L
from .tape import Tape


def _ptr(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


def _f32(t: torch.Tensor, device) -> torch.Tensor:
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def timesteps(t, batch: int):
    """The one rule for a timestep argument of a call on `batch` samples.  A scalar, a 0-d or a 1-element t is shared by the batch: returns the
    float.  A t of exactly `batch` elements is per-sample: returns the list of floats, collapsed to the one float when they are all equal.  Any
    other length raises ValueError (the batch would silently run at t[0])."""
    if torch.is_tensor(t):
        v = [float(a) for a in t.detach().reshape(-1).to(torch.float32).tolist()]
    elif isinstance(t, (list, tuple)):
        v = [float(torch.tensor(a, dtype=torch.float32).item()) for a in t]
    else:
        v = [float(torch.tensor(t, dtype=torch.float32).item())]
    if len(v) != 1 and len(v) != int(batch):
        raise ValueError(f"timestep has {len(v)} elements for a batch of {batch}: one (shared by the batch) or one per sample")
    return v[0] if all(a == v[0] for a in v) else v


class Engine:
    def __init__(self, tape: Tape, temb_dim: int, flip_sin_to_cos: bool, half_minus_one: bool, x_channels: int,
                 max_batch: int = 1, max_tangents: int = 16):
        self.lib = L.load()
        if tape.device.type != "cuda":
            raise L.DpbError("the pullback engine needs a HIP device (there is no CPU fallback)")
        self.tape = tape
        self.device = tape.device
        self.max_batch, self.max_tangents = max_batch, max_tangents
        self.x_channels = x_channels
        nb, no = len(tape.buffers), len(tape.ops)
        self._bufs = (L.BufferDesc * nb)(*[L.BufferDesc(r, c, k, v) for (r, c, k), v in zip(tape.buffers, tape.valid)])
        ops = (L.OpDesc * no)()
        for i, d in enumerate(tape.ops):
            o = ops[i]
            o.kind, o.in0, o.in1, o.in2, o.out, o.res, o.rowbias = d["kind"], d["in0"], d["in1"], d["in2"], d["out"], d["res"], d["rowbias"]
            for j in range(12):
                o.ip[j] = int(d["ip"][j])
            for j in range(4):
                o.fp[j] = float(d["fp"][j])
                o.w[j] = d["w"][j] or None
        self._ops = ops
        net = L.NetDesc()
        net.dtype = L.dtype_code(tape.dtype)
        net.max_batch, net.max_tangents = max_batch, max_tangents
        net.n_buffers, net.n_ops = nb, no
        net.buffers, net.ops = self._bufs, self._ops
        net.x_buf, net.x_channels = tape.x, x_channels
        net.temb_buf, net.temb_dim = tape.temb_in, temb_dim
        net.temb_flip_sin_to_cos, net.temb_half_minus_one = int(flip_sin_to_cos), int(half_minus_one)
        net.ctx_buf = getattr(tape, "ctx", -1)
        self._net = net
        h = C.c_void_p()
        L.check(self.lib.dpb_engine_create(C.byref(net), C.byref(h)))
        self.h = h
        self.ws_bytes = int(self.lib.dpb_engine_workspace_bytes(h))
        with torch.cuda.device(self.device):
            self._ws = torch.empty(self.ws_bytes + 256, dtype=torch.uint8, device=self.device)
            off = (-self._ws.data_ptr()) % 256
            self._set_stream()
            L.check(self.lib.dpb_engine_set_workspace(h, C.c_void_p(self._ws.data_ptr() + off), self.ws_bytes))
        self.x_rows = tape.buffers[tape.x][0]
        self.n_in = self.x_rows * x_channels
        self.batch = 0

    def __del__(self):
        try:
            if getattr(self, "h", None):
                torch.cuda.synchronize(self.device)
                self.lib.dpb_engine_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def _set_stream(self):
        s = torch.cuda.current_stream(self.device).cuda_stream
        L.check(self.lib.dpb_engine_set_stream(self.h, C.c_void_p(s)))
        return s

    # ------------------------------------------------------------------ passes
    def tap_numel(self, tap) -> int:
        c, h, w = self.tape.tap_shape[self.tape.taps[tap]]
        return c * h * w

    def _directions(self, u: torch.Tensor, tap, empty_ok: bool = False) -> torch.Tensor:
        """u as fp32 [nu, N_tap] on the device: a whole number of NCHW-flattened directions of `tap` (empty_ok: nu = 0 is left to the library)"""
        d = self.tap_numel(tap)
        if (u.numel() == 0 and not empty_ok) or u.numel() % d:
            raise L.DpbError(f"u has {u.numel()} elements, not a whole number of directions of {d} (tap {tap})")
        return _f32(u, self.device).reshape(-1, d)

    def _scratch(self, need: int):
        """a 256-byte aligned pointer to `need` bytes of the engine's one grow-only device scratch; the calls that use it run on the engine's one
        stream, one after the other"""
        if getattr(self, "_scratch_buf", None) is None or self._scratch_buf.numel() < need + 256:
            self._scratch_buf = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
        return C.c_void_p(self._scratch_buf.data_ptr() + (-self._scratch_buf.data_ptr()) % 256)

    def _inputs(self, x: torch.Tensor, ctx: Optional[torch.Tensor]):
        x = _f32(x, self.device)
        b = x.shape[0]
        if x[0].numel() != self.n_in:
            raise L.DpbError(f"input has {x[0].numel()} elements per sample, network expects {self.n_in}")
        cbuf = getattr(self.tape, "ctx", -1)
        if cbuf >= 0:
            if ctx is None:
                raise L.DpbError("this network needs encoder_hidden_states (ctx)")
            rows, cpad, _ = self.tape.buffers[cbuf]
            width = self.tape.valid[cbuf] or cpad
            if ctx.dim() != 3 or ctx.shape[1] != rows or ctx.shape[2] != width or ctx.shape[0] not in (1, b):
                raise L.DpbError(f"encoder_hidden_states has shape {tuple(ctx.shape)}, the engine was built for [{b} or 1, {rows}, {width}] "
                                 "(token count and width are fixed at engine build time: SDConfig.ctx_len / cross_dim)")
            ctx = _f32(ctx, self.device)
            if ctx.shape[0] != b:
                ctx = ctx.expand(b, -1, -1).contiguous()
        else:
            ctx = None
        return x, b, ctx

    def primal(self, x: torch.Tensor, t, ctx: Optional[torch.Tensor], tap) -> None:
        """x [B,C,H,W]; ctx [B,L,D] or None; t a float, or a sequence / tensor of B timesteps (row b is the net at t[b]: dpb_primal_t).
        Keeps the activations resident for jvp/vjp."""
        buf = self.tape.taps[tap]
        with torch.cuda.device(self.device):
            self._set_stream()
            x, b, ctx = self._inputs(x, ctx)
            t = timesteps(t, b)
            if isinstance(t, float):
                L.check(self.lib.dpb_primal(self.h, _ptr(x), b, t, _ptr(ctx), buf))
            else:
                L.check(self.lib.dpb_primal_t(self.h, _ptr(x), b, (C.c_float * b)(*t), _ptr(ctx), buf))
            self.batch = b

    def read(self, tap) -> torch.Tensor:
        buf = self.tape.taps[tap]
        c, h, w = self.tape.tap_shape[buf]
        if self.batch < 1:
            raise L.DpbError("no primal state to read: forward() keeps none (dpb_forward); call primal() first")
        with torch.cuda.device(self.device):
            self._set_stream()
            out = torch.empty(self.batch, c, h, w, dtype=torch.float32, device=self.device)
            L.check(self.lib.dpb_read_buffer(self.h, buf, c, _ptr(out)))
        return out

    def forward(self, x, t, ctx=None, tap="eps", out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Forward only (dpb_forward): the U-Net calls of the DDIM / guidance loop and get_h.  Keeps no tangent / adjoint stash,
        so jvp / vjp / iterate need a primal() first (the engine refuses otherwise).  out: a contiguous fp32 device tensor of
        B * C * H * W elements to write into (a row slice of a feature matrix); returned viewed as [B, C, H, W].  t: a float, or a sequence /
        tensor of B timesteps (dpb_forward_t)."""
        buf = self.tape.taps[tap]
        c, h, w = self.tape.tap_shape[buf]
        with torch.cuda.device(self.device):
            self._set_stream()
            x, b, ctx = self._inputs(x, ctx)
            if out is None:
                out = torch.empty(b, c, h, w, dtype=torch.float32, device=self.device)
            else:
                if not (out.is_cuda and out.device == x.device and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == b * c * h * w):
                    raise L.DpbError(f"out must be a contiguous fp32 tensor of {b * c * h * w} elements on {x.device}")
                out = out.view(b, c, h, w)
            t = timesteps(t, b)
            if isinstance(t, float):
                L.check(self.lib.dpb_forward(self.h, _ptr(x), b, t, _ptr(ctx), buf, c, _ptr(out)))
            else:
                L.check(self.lib.dpb_forward_t(self.h, _ptr(x), b, (C.c_float * b)(*t), _ptr(ctx), buf, c, _ptr(out)))
            self.batch = 0
        return out

    def jvp(self, tap, V: torch.Tensor) -> torch.Tensor:
        """V [nt, N_in] (NCHW-flattened) -> U [nt, N_h]"""
        buf = self.tape.taps[tap]
        with torch.cuda.device(self.device):
            self._set_stream()
            V = _f32(V, self.device).reshape(-1, self.n_in)
            U = torch.empty(V.shape[0], self.tap_numel(tap), dtype=torch.float32, device=self.device)
            L.check(self.lib.dpb_jvp(self.h, buf, _ptr(V), V.shape[0], _ptr(U)))
        return U

    def vjp(self, tap, U: torch.Tensor) -> torch.Tensor:
        buf = self.tape.taps[tap]
        with torch.cuda.device(self.device):
            self._set_stream()
            U = _f32(U, self.device).reshape(-1, self.tap_numel(tap))
            W = torch.empty(U.shape[0], self.n_in, dtype=torch.float32, device=self.device)
            L.check(self.lib.dpb_vjp(self.h, buf, _ptr(U), U.shape[0], _ptr(W)))
        return W

    def orth(self, W: torch.Tensor, Vprev: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        with torch.cuda.device(self.device):
            s_ = self._set_stream()
            W = _f32(W, self.device); Vprev = _f32(Vprev, self.device)
            k, n = W.shape
            V = torch.empty_like(W)
            s = torch.empty(k, dtype=torch.float32, device=self.device)
            conv = torch.empty(2, dtype=torch.float32, device=self.device)
            scratch = torch.empty(int(self.lib.dpb_orth_scratch_bytes(k, n)) // 8 + 1, dtype=torch.float64, device=self.device)
            L.check(self.lib.dpb_orth_checked(_ptr(W), _ptr(Vprev), _ptr(V), _ptr(s), _ptr(conv), _ptr(scratch), scratch.numel() * 8, k, n, C.c_void_p(s_)))
        return V, s, conv

    def iterate(self, tap, V: torch.Tensor, n_iters: int):
        """n_iters power iterations in place on V [B*k, N_in] (B = batch of the last primal, independent bases);
        returns (V, U [B*k, N_h], s [B*k], conv [B, 2]) device tensors, no host sync."""
        buf = self.tape.taps[tap]
        with torch.cuda.device(self.device):
            self._set_stream()
            assert V.is_cuda and V.dtype == torch.float32 and V.is_contiguous() and V.shape[0] % self.batch == 0
            nt = V.shape[0]
            k = nt // self.batch
            U = torch.empty(nt, self.tap_numel(tap), dtype=torch.float32, device=self.device)
            s = torch.empty(nt, dtype=torch.float32, device=self.device)
            conv = torch.empty(self.batch, 2, dtype=torch.float32, device=self.device)
            L.check(self.lib.dpb_pullback_iterate(self.h, buf, _ptr(V), _ptr(U), _ptr(s), _ptr(conv), k, n_iters))
        return V, U, s, conv

    # ------------------------------------------------------------------ passes seeded at a tap (the decoder Jacobian d dst / d src)
    def forward_from(self, x: torch.Tensor, t: float, ctx: Optional[torch.Tensor], src, h: torch.Tensor, dst="eps") -> torch.Tensor:
        """dpb_forward_from: the forward pass with the activation at tap `src` replaced by h [B, C, H, W] (x [B, ...]: the caller repeats
        one sample), read at `dst`.  Like forward(), keeps no primal state."""
        sbuf, dbuf = self.tape.taps[src], self.tape.taps[dst]
        c, hh, ww = self.tape.tap_shape[dbuf]
        with torch.cuda.device(self.device):
            self._set_stream()
            x, b, ctx = self._inputs(x, ctx)
            h = _f32(h, self.device).reshape(b, -1)
            if h.shape[1] != self.tap_numel(src):
                raise L.DpbError(f"input_h has {h.shape[1]} elements per sample, tap {src} has {self.tap_numel(src)}")
            out = torch.empty(b, c, hh, ww, dtype=torch.float32, device=self.device)
            L.check(self.lib.dpb_forward_from(self.h, _ptr(x), b, float(t), _ptr(ctx), sbuf, _ptr(h), dbuf, c, _ptr(out)))
            self.batch = 0
        return out

    def forward_shift(self, x: torch.Tensor, t: float, ctx: Optional[torch.Tensor], src, u: torch.Tensor, dirs, scales, dst="eps") -> torch.Tensor:
        """dpb_forward_shift: row b of the result is `dst` of the net with the activation at tap `src` replaced by h(x_b) + scales[b] * u[dirs[b]]
        (dirs[b] = -1: unshifted).  u [nu, N_src] fp32 directions (NCHW-flattened; a device tensor is used where it lies), dirs / scales: host
        sequences of B entries.  x [B, ...] (ctx [B or 1, L, D]): one forward pass at B; x [1, ...] with B > 1: the shared prefix -- the part of
        the net up to the tap runs once, only the part after it at B.  Like forward(), keeps no primal state."""
        dirs, scales = [int(d) for d in dirs], [float(s) for s in scales]
        b = len(dirs)
        if len(scales) != b:
            raise L.DpbError(f"dirs has {b} entries, scales {len(scales)}: one of each per output row")
        return self._shifted(self.lib.dpb_forward_shift, b, lambda xb: b, True, x, t, ctx, src, u, dirs, scales, dst)

    def _shifted(self, call, second, rows, empty_ok, x, t, ctx, src, u, dirs, scales, dst) -> torch.Tensor:
        """forward_shift and forward_shift_groups behind their own checks: `call` is the entry point, `second` its argument after xbatch (the batch,
        or the groups), rows(xb) the number of output rows, raising where dirs / scales do not fit it; empty_ok: see _directions"""
        sbuf, dbuf = self.tape.taps[src], self.tape.taps[dst]
        c, hh, ww = self.tape.tap_shape[dbuf]
        with torch.cuda.device(self.device):
            self._set_stream()
            x, xb, ctx = self._inputs(x, ctx)
            b = rows(xb)
            u = self._directions(u, src, empty_ok)
            out = torch.empty(max(b, 1), c, hh, ww, dtype=torch.float32, device=self.device)
            self.batch = 0
            L.check(call(self.h, _ptr(x), xb, second, float(t), _ptr(ctx), sbuf, _ptr(u), u.shape[0], (C.c_int32 * max(b, 1))(*dirs),
                         (C.c_float * max(b, 1))(*scales), dbuf, c, _ptr(out)))
        return out

    def jvp_between(self, src, dst, V: torch.Tensor) -> torch.Tensor:
        """V [nt, N_src] (NCHW-flattened tangents of the tap `src`) -> U [nt, N_dst]; the primal must reach `dst`"""
        with torch.cuda.device(self.device):
            self._set_stream()
            V = _f32(V, self.device).reshape(-1, self.tap_numel(src))
            U = torch.empty(V.shape[0], self.tap_numel(dst), dtype=torch.float32, device=self.device)
            L.check(self.lib.dpb_jvp_between(self.h, self.tape.taps[src], self.tape.taps[dst], _ptr(V), V.shape[0], _ptr(U)))
        return U

    def vjp_between(self, src, dst, U: torch.Tensor) -> torch.Tensor:
        """U [nt, N_dst] -> W = J^T U [nt, N_src]"""
        with torch.cuda.device(self.device):
            self._set_stream()
            U = _f32(U, self.device).reshape(-1, self.tap_numel(dst))
            W = torch.empty(U.shape[0], self.tap_numel(src), dtype=torch.float32, device=self.device)
            L.check(self.lib.dpb_vjp_between(self.h, self.tape.taps[src], self.tape.taps[dst], _ptr(U), U.shape[0], _ptr(W)))
        return W

    def scratch_bytes(self, src, k: int) -> int:
        """device scratch of iterate_between for k directions per sample (dpb_pullback_scratch_bytes, at max_batch)"""
        return int(self.lib.dpb_pullback_scratch_bytes(self.h, self.tape.taps[src], int(k)))

    def iterate_between(self, src, dst, V: torch.Tensor, n_iters: int, scratch: Optional[torch.Tensor] = None):
        """iterate() between two taps: n_iters power iterations in place on V [B*k, N_src]; returns (V, U [B*k, N_dst], s [B*k], conv [B, 2]).
        scratch: uint8 device tensor of >= scratch_bytes(src, k) + 256 bytes (allocated here when None)."""
        with torch.cuda.device(self.device):
            self._set_stream()
            assert V.is_cuda and V.dtype == torch.float32 and V.is_contiguous() and self.batch > 0 and V.shape[0] % self.batch == 0
            nt = V.shape[0]
            k = nt // self.batch
            need = self.scratch_bytes(src, k)
            if scratch is None:
                scratch = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
            off = (-scratch.data_ptr()) % 256
            U = torch.empty(nt, self.tap_numel(dst), dtype=torch.float32, device=self.device)
            s = torch.empty(nt, dtype=torch.float32, device=self.device)
            conv = torch.empty(self.batch, 2, dtype=torch.float32, device=self.device)
            L.check(self.lib.dpb_pullback_iterate_between(self.h, self.tape.taps[src], self.tape.taps[dst], _ptr(V), _ptr(U), _ptr(s), _ptr(conv), k,
                                                          n_iters, C.c_void_p(scratch.data_ptr() + off), max(scratch.numel() - off, 0)))
        return V, U, s, conv

    # ------------------------------------------------------------------ local PCA: the sampling loop on the device
    def local_pca_sample(self, x: torch.Tensor, t: float, ctx: Optional[torch.Tensor], tap, count: int, noise: Optional[torch.Tensor] = None,
                         seed: int = 0, first: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """dpb_local_pca_sample: `count` feature rows get_h(x + g_i / ||g_i||), i = first .. first + count - 1, of ONE input x [1, C, H, W]
        (ctx [1, L, D] or None) at `tap`, in chunks of max_batch with no host round trip per chunk.  g_i = noise[i - first] (noise [count, ...]
        unnormalised Gaussian draws) or, when noise is None, generated on the device from (seed, i).  out: a contiguous fp32 [count, D] device
        tensor to write into (rows of a larger matrix), allocated here when None.  Like forward(), keeps no primal state."""
        buf = self.tape.taps[tap]
        c, h, w = self.tape.tap_shape[buf]
        d = c * h * w
        count, first = int(count), int(first)
        with torch.cuda.device(self.device):
            self._set_stream()
            x, b, ctx = self._inputs(x, ctx)
            if b != 1:
                raise L.DpbError(f"local_pca_sample perturbs ONE input, got a batch of {b}")
            if count < 1 or first < 0:
                raise L.DpbError(f"local_pca_sample: count={count} and first={first} must be >= 1 and >= 0")
            if noise is not None:
                if noise.numel() != count * self.n_in:
                    raise L.DpbError(f"noise has {noise.numel()} elements, expected count * N_in = {count} * {self.n_in}")
                noise = _f32(noise, self.device)
            if out is None:
                out = torch.empty(count, d, dtype=torch.float32, device=self.device)
            elif not (out.is_cuda and out.device == x.device and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == count * d):
                raise L.DpbError(f"out must be a contiguous fp32 tensor of {count * d} elements on {x.device}")
            need = int(self.lib.dpb_local_pca_scratch_bytes(self.h))
            self.batch = 0
            L.check(self.lib.dpb_local_pca_sample(self.h, _ptr(x), float(t), _ptr(ctx), buf, c, _ptr(noise), C.c_uint64(int(seed) & (2 ** 64 - 1)), first,
                                                  count, _ptr(out), self._scratch(need), need))
        return out.view(count, d)

    # ------------------------------------------------------------------ the parallel-h edit chain on the device
    def inv_jac_chain(self, x: torch.Tensor, t, ctx: Optional[torch.Tensor], tap, u: torch.Tensor, dirs, signs, step, steps: int,
                      sega_sigma: float = 0.0, final_shift: bool = True, return_vk: bool = False):
        """dpb_inv_jac_chain: n = x.shape[0] chains advanced together for `steps` steps with no Python between the steps.  x [n, C, H, W], t a float
        or n timesteps, ctx [n or 1, L, D] or None, u [nu, N_h] fp32 directions of `tap` (NCHW-flattened), dirs / signs / step: host sequences of n
        entries (chain b follows signs[b] * u[dirs[b]] with step[b] per step; each step moves x along -J^T c / ||J^T c||).  Returns device tensors
        (states [steps + 1, n, C, H, W], vk [steps, n, N_in] or None, stats [steps, n, 4] fp64 = (||J^T c||^2, SEGA std, elements kept, flag),
        shift [steps + 1, n, 2] fp64 = (<h - h0, c> / ||c||, ||h - h0||^2)); no host sync beyond the one of the first primal pass.  Like forward(),
        keeps no primal state."""
        buf = self.tape.taps[tap]
        steps = int(steps)
        with torch.cuda.device(self.device):
            self._set_stream()
            x, n, ctx = self._inputs(x, ctx)
            tl = timesteps(t, n)
            tl = [tl] * n if isinstance(tl, float) else tl
            dirs, signs, step = [int(d) for d in dirs], [float(s) for s in signs], [float(s) for s in step]
            if not (len(dirs) == len(signs) == len(step) == n):
                raise L.DpbError(f"dirs, signs and step have {len(dirs)}, {len(signs)} and {len(step)} entries for {n} chains: one of each per chain")
            u = self._directions(u, tap)
            ns = max(steps, 1)
            states = torch.empty(ns + 1, n, *x.shape[1:], dtype=torch.float32, device=self.device)
            vk = torch.empty(ns, n, self.n_in, dtype=torch.float32, device=self.device) if return_vk else None
            stats = torch.empty(ns, n, 4, dtype=torch.float64, device=self.device)
            shift = torch.empty(ns + 1, n, 2, dtype=torch.float64, device=self.device)
            need = int(self.lib.dpb_inv_jac_chain_scratch_bytes(self.h, buf, n))
            self.batch = 0
            L.check(self.lib.dpb_inv_jac_chain(self.h, buf, _ptr(x), n, (C.c_float * n)(*tl), _ptr(ctx), _ptr(u), u.shape[0], (C.c_int32 * n)(*dirs),
                                               (C.c_float * n)(*signs), (C.c_float * n)(*step), steps, float(sega_sigma), int(bool(final_shift)),
                                               _ptr(states), _ptr(vk), _ptr(stats), _ptr(shift), self._scratch(need), need))
        return states, vk, stats, shift

    # ------------------------------------------------------------------ the least-squares inverse of the Jacobian and the newton-h chain
    def jac_lstsq(self, tap, c: torch.Tensor, mu_abs: float = 0.0, mu_rel: float = 0.1, tol: float = 1e-5, iters: int = 16,
                  return_resid: bool = False):
        """dpb_jac_lstsq on the state primal() left: CGLS on min ||J d - c||^2 + mu ||d||^2 from d = 0, per row, mu = mu_abs + mu_rel ||J^T c||^2 /
        ||c||^2.  c [nt, N_h] (NCHW-flattened), with jvp()'s row convention: row j belongs to sample j // (nt // batch).  Returns device tensors
        (delta [nt, N_in], resid [nt, N_h] or None, hist [iters + 1, nt, 4] fp64 = (gamma, ||r||^2, ||d||^2, flag)); no host sync; the primal state
        stays usable (include/dpb.h states the recurrence and the flags)."""
        buf = self.tape.taps[tap]
        iters = int(iters)
        with torch.cuda.device(self.device):
            self._set_stream()
            c = _f32(c, self.device).reshape(-1, self.tap_numel(tap))
            nt = c.shape[0]
            delta = torch.empty(nt, self.n_in, dtype=torch.float32, device=self.device)
            resid = torch.empty_like(c) if return_resid else None
            hist = torch.empty(max(iters, 0) + 1, nt, 4, dtype=torch.float64, device=self.device)
            need = int(self.lib.dpb_jac_lstsq_scratch_bytes(self.h, buf, nt))
            L.check(self.lib.dpb_jac_lstsq(self.h, buf, _ptr(c), nt, float(mu_abs), float(mu_rel), float(tol), iters, _ptr(delta), _ptr(resid),
                                           _ptr(hist), self._scratch(need), need))
        return delta, resid, hist

    def newton_h_chain(self, x: torch.Tensor, t, ctx: Optional[torch.Tensor], tap, u: torch.Tensor, dirs, signs, scale, steps: int, iters: int,
                       mu_abs: float = 0.0, mu_rel: float = 0.1, tol: float = 1e-5, radius: float = 0.0, final_shift: bool = True):
        """dpb_newton_h_chain: n = x.shape[0] damped Gauss-Newton chains advanced together, chain b towards h0_b + scale[b] * signs[b] * u[dirs[b]]
        in `steps` outer steps of `iters` CGLS iterations each, with no Python between them.  A chain with sign +1 moves h ALONG its direction (the
        opposite of inv_jac_chain).  Returns device tensors (states [steps + 1, n, C, H, W], hist [steps, iters + 1, n, 4] fp64, step_stats
        [steps, n, 4] fp64 = (||res||^2, ||delta||^2, kappa, flag), shift [steps + 1, n, 2] fp64 as inv_jac_chain's).  Like forward(), keeps no
        primal state."""
        buf = self.tape.taps[tap]
        steps, iters = int(steps), int(iters)
        with torch.cuda.device(self.device):
            self._set_stream()
            x, n, ctx = self._inputs(x, ctx)
            tl = timesteps(t, n)
            tl = [tl] * n if isinstance(tl, float) else tl
            dirs, signs, scale = [int(d) for d in dirs], [float(s) for s in signs], [float(s) for s in scale]
            if not (len(dirs) == len(signs) == len(scale) == n):
                raise L.DpbError(f"dirs, signs and scale have {len(dirs)}, {len(signs)} and {len(scale)} entries for {n} chains: one of each per chain")
            u = self._directions(u, tap)
            ns, ni = max(steps, 1), max(iters, 0)
            states = torch.empty(ns + 1, n, *x.shape[1:], dtype=torch.float32, device=self.device)
            hist = torch.empty(ns, ni + 1, n, 4, dtype=torch.float64, device=self.device)
            step_stats = torch.empty(ns, n, 4, dtype=torch.float64, device=self.device)
            shift = torch.empty(ns + 1, n, 2, dtype=torch.float64, device=self.device)
            need = int(self.lib.dpb_newton_h_chain_scratch_bytes(self.h, buf, n))
            self.batch = 0
            L.check(self.lib.dpb_newton_h_chain(self.h, buf, _ptr(x), n, (C.c_float * n)(*tl), _ptr(ctx), _ptr(u), u.shape[0], (C.c_int32 * n)(*dirs),
                                                (C.c_float * n)(*signs), (C.c_float * n)(*scale), steps, iters, float(mu_abs), float(mu_rel), float(tol),
                                                float(radius), int(bool(final_shift)), _ptr(states), _ptr(hist), _ptr(step_stats), _ptr(shift),
                                                self._scratch(need), need))
        return states, hist, step_stats, shift

    # ------------------------------------------------------------------ the h-space guidance edit on the device
    def forward_shift_groups(self, x: torch.Tensor, groups: int, t: float, ctx: Optional[torch.Tensor], src, u: torch.Tensor, dirs, scales,
                             dst="eps") -> torch.Tensor:
        """dpb_forward_shift_groups: forward_shift for `groups` shifted copies of the xb = x.shape[0] DIFFERENT samples of x.  Row g * xb + b of
        the result is `dst` of sample b with scales[g * xb + b] * u[dirs[g * xb + b]] added at tap `src` (dirs = -1: unshifted); dirs / scales:
        host sequences of xb * groups entries.  The part of the net up to the tap runs once at xb, the part after it at xb * groups.  Like
        forward(), keeps no primal state."""
        dirs, scales, groups = [int(d) for d in dirs], [float(s) for s in scales], int(groups)

        def rows(xb):
            if len(dirs) != xb * max(groups, 0) or len(scales) != xb * max(groups, 0):
                raise L.DpbError(f"dirs and scales have {len(dirs)} and {len(scales)} entries for {xb} samples x {groups} groups: one of each per row")
            return xb * max(groups, 0)
        return self._shifted(self.lib.dpb_forward_shift_groups, groups, rows, False, x, t, ctx, src, u, dirs, scales, dst)

    def hguide_chain(self, x: torch.Tensor, t, alpha_t, alpha_next, ctx: Optional[torch.Tensor], tap, u: torch.Tensor, dirs, scales, gP: float = 1.0,
                     gD: float = 0.0):
        """dpb_hguide_chain: n = x.shape[0] chains advanced together through the S = len(t) DDIM steps (t[j], alpha_t[j]) -> alpha_next[j] with no
        Python between the steps; chain b adds scales[b] * u[dirs[b]] at `tap` in the shifted row of every step.  t / alpha_t / alpha_next: host
        sequences of S floats (the fp32 table entries), ctx [n or 1, L, D] or None, u [nu, N_h] fp32 (NCHW-flattened), dirs / scales: host
        sequences of n.  2n rows run per step: n <= max_batch // 2.  Returns device tensors (states [S + 1, n, C, H, W] with states[0] = x,
        delta [S, n, 2] fp64 = (||e_s - e||^2, flag)); one host sync for the call.  Like forward(), keeps no primal state."""
        buf, ebuf = self.tape.taps[tap], self.tape.taps["eps"]
        tl, al, an = [float(a) for a in t], [float(a) for a in alpha_t], [float(a) for a in alpha_next]
        steps = len(tl)
        if len(al) != steps or len(an) != steps:
            raise L.DpbError(f"t, alpha_t and alpha_next have {steps}, {len(al)} and {len(an)} entries: one of each per step")
        with torch.cuda.device(self.device):
            self._set_stream()
            x, n, ctx = self._inputs(x, ctx)
            dirs, scales = [int(d) for d in dirs], [float(s) for s in scales]
            if len(dirs) != n or len(scales) != n:
                raise L.DpbError(f"dirs and scales have {len(dirs)} and {len(scales)} entries for {n} chains: one of each per chain")
            u = self._directions(u, tap)
            ns = max(steps, 1)
            states = torch.empty(ns + 1, n, *x.shape[1:], dtype=torch.float32, device=self.device)
            delta = torch.empty(ns, n, 2, dtype=torch.float64, device=self.device)
            need = int(self.lib.dpb_hguide_chain_scratch_bytes(self.h, n, ns))
            self.batch = 0
            fa = C.c_float * ns
            L.check(self.lib.dpb_hguide_chain(self.h, buf, ebuf, _ptr(x), n, fa(*tl), fa(*al), fa(*an), _ptr(ctx), _ptr(u), u.shape[0],
                                              (C.c_int32 * n)(*dirs), (C.c_float * n)(*scales), float(gP), float(gD), steps, _ptr(states), _ptr(delta),
                                              self._scratch(need), need))
        return states, delta

    # ------------------------------------------------------------------ pullback geodesics between two latents on the device
    def geodesic_chain(self, P: torch.Tensor, t: float, ctx: Optional[torch.Tensor], tap, eta: float, lam: float, iters: int,
                       final_energy: bool = True):
        """dpb_geodesic_chain: `iters` Jacobi iterations P_i <- P_i - eta (J(P_i)^T (2 h_i - h_{i-1} - h_{i+1}) + lam (2 P_i - P_{i-1} - P_{i+1}))
        of the m = P.shape[0] - 2 interior points of the curve P [m + 2, C, H, W] with no Python between them; the end rows stay.  One timestep t;
        ctx [m + 2 or 1, L, D] or None.  Returns device tensors (curves [iters + 1, m + 2, C, H, W] with curves[0] = P, seg_h and seg_x
        [iters + 1, m + 1] fp64 = ||h_{i+1} - h_i||^2 and ||P_{i+1} - P_i||^2 of every curve (the last row NaN unless final_energy, which takes one
        more forward pass), stats [iters, m, 4] fp64 = (||J^T c||^2, ||g||^2, ||P_out - P||^2, flag), csq [iters, m] fp64 = ||c_i||^2); one host
        sync for the call.  Like forward(), keeps no primal state."""
        buf = self.tape.taps[tap]
        iters = int(iters)
        with torch.cuda.device(self.device):
            self._set_stream()
            P, n, ctx = self._inputs(P, ctx)
            m = n - 2
            ni, nm = max(iters, 1), max(m, 1)
            curves = torch.empty(ni + 1, nm + 2, *P.shape[1:], dtype=torch.float32, device=self.device)
            seg_h = torch.empty(ni + 1, nm + 1, dtype=torch.float64, device=self.device)
            seg_x = torch.empty(ni + 1, nm + 1, dtype=torch.float64, device=self.device)
            stats = torch.empty(ni, nm, 4, dtype=torch.float64, device=self.device)
            csq = torch.empty(ni, nm, dtype=torch.float64, device=self.device)
            need = int(self.lib.dpb_geodesic_chain_scratch_bytes(self.h, buf, m))
            self.batch = 0
            L.check(self.lib.dpb_geodesic_chain(self.h, buf, _ptr(P), m, float(t), _ptr(ctx), float(eta), float(lam), iters, int(bool(final_energy)),
                                                _ptr(curves), _ptr(seg_h), _ptr(seg_x), _ptr(stats), _ptr(csq), self._scratch(need), need))
        return curves, seg_h, seg_x, stats, csq

    def profile(self, enable: bool):
        L.check(self.lib.dpb_engine_profile(self.h, int(enable)))

    def profile_dump(self, path: str):
        L.check(self.lib.dpb_engine_profile_dump(self.h, path.encode()))

    def profile_read(self, big_tile: int):
        n = C.c_int64(); ms = C.c_double(); f = C.c_double()
        L.check(self.lib.dpb_engine_profile_read(self.h, int(big_tile), C.byref(n), C.byref(ms), C.byref(f)))
        return n.value, ms.value, f.value

    def profile_overhead_ms(self) -> float:
        """the calibrated empty-bracket time subtracted from every launch of profile_read / profile_dump"""
        v = C.c_double()
        L.check(self.lib.dpb_engine_profile_overhead(self.h, C.byref(v)))
        return v.value

    def stats(self):
        n = C.c_int64(); f = C.c_double(); b = C.c_double()
        L.check(self.lib.dpb_engine_stats(self.h, C.byref(n), C.byref(f), C.byref(b)))
        return n.value, f.value, b.value


def pca_lowrank(H: torch.Tensor, R: torch.Tensor, q: int, niter: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """torch.pca_lowrank(H, q, center=True, niter) on the GPU (dpb_pca_lowrank; engine-independent).  H [N, D] fp32 contiguous on a HIP device,
    R the Gaussian draw of torch._lowrank.get_approximate_basis ([N, q] if N < D, else [D, q]).  Returns device tensors u [q, D] (rows = the
    columns of pca_lowrank's V, sign arbitrary) and s [q]; no host sync.  Limits: 1 <= q <= 128, q <= N - 1, q <= D."""
    lib = L.load()
    if H.dim() != 2 or not H.is_cuda or H.dtype != torch.float32 or not H.is_contiguous():
        raise L.DpbError("H must be a contiguous fp32 [N, D] tensor on a HIP device")
    n, d = H.shape
    with torch.cuda.device(H.device):
        st = torch.cuda.current_stream(H.device).cuda_stream
        need = int(lib.dpb_pca_scratch_bytes(int(q), n, d))
        R = _f32(R, H.device)
        u = torch.empty(max(int(q), 1), d, dtype=torch.float32, device=H.device)
        s = torch.empty(max(int(q), 1), dtype=torch.float32, device=H.device)
        if need == 0:                                  # unsupported shape: the library states why
            L.check(lib.dpb_pca_lowrank(_ptr(H), n, d, _ptr(R), int(q), int(niter), _ptr(u), _ptr(s), None, 0, C.c_void_p(st)))
        if tuple(R.shape) != (min(n, d), q):
            raise L.DpbError(f"R has shape {tuple(R.shape)}, expected [{min(n, d)}, {q}] (torch.randn(A.shape[-1], q) of _svd_lowrank's A)")
        scratch = torch.empty(need, dtype=torch.uint8, device=H.device)
        L.check(lib.dpb_pca_lowrank(_ptr(H), n, d, _ptr(R), int(q), int(niter), _ptr(u), _ptr(s), _ptr(scratch), need, C.c_void_p(st)))
    return u, s


def perturb_unit(x: torch.Tensor, B: int, noise: Optional[torch.Tensor] = None, seed: int = 0, first: int = 0, norm: float = 1.0,
                 return_noise: bool = False):
    """dpb_perturb_unit (engine-independent): out[b] = x + norm * g_b / ||g_b||_2 for b < B, x one fp32 input of any shape on a HIP device,
    g_b = noise[b] (noise [B, *x.shape]) or the kernel's Philox4x32-10 normals of (seed, first + b) (include/dpb.h states the mapping).
    Returns out [B, n] (n = x.numel()), and the unnormalised g [B, n] as well when return_noise.  No host sync."""
    lib = L.load()
    if not x.is_cuda:
        raise L.DpbError("x must be on a HIP device")
    x = _f32(x, x.device).reshape(-1)
    n, B = x.numel(), int(B)
    with torch.cuda.device(x.device):
        st = torch.cuda.current_stream(x.device).cuda_stream
        if noise is not None:
            if noise.numel() != B * n:
                raise L.DpbError(f"noise has {noise.numel()} elements, expected B * n = {B} * {n}")
            noise = _f32(noise, x.device)
        out = torch.empty(max(B, 1), n, dtype=torch.float32, device=x.device)
        g = torch.empty(max(B, 1), n, dtype=torch.float32, device=x.device) if return_noise else None
        need = int(lib.dpb_perturb_scratch_bytes(B, n))
        scratch = torch.empty(max(need // 8, 1), dtype=torch.float64, device=x.device)
        L.check(lib.dpb_perturb_unit(_ptr(x), _ptr(noise), C.c_uint64(int(seed) & (2 ** 64 - 1)), int(first), B, n, float(norm), _ptr(out), _ptr(g),
                                     _ptr(scratch), need, C.c_void_p(st)))
    return (out, g) if return_noise else out


def direction_step(W: torch.Tensor, x: torch.Tensor, step, sega_sigma: float = 0.0, out: Optional[torch.Tensor] = None, return_vk: bool = True):
    """dpb_direction_step (engine-independent): per row b of W [n, N] (the adjoint results J^T c) and x [n, N], fp32 on a HIP device,
    v = -W_b / ||W_b||, the SEGA rule v <- where(|v| < sega_sigma * std(v), 0, v) when sega_sigma > 0, x_out = x + step[b] * v.  step: a float or a
    host sequence of n.  out: the tensor x_out is written into (x itself for an in-place step), allocated here when None.  Returns (x_out, vk or
    None, stats [n, 4] fp64 = (||W_b||^2, std or 0, elements kept, flag)); a zero or non-finite row has its flag set and NaN in its row of x_out
    and vk.  No host sync (include/dpb.h states the arithmetic)."""
    lib = L.load()
    if not (W.is_cuda and W.dim() == 2 and W.dtype == torch.float32 and W.is_contiguous()):
        raise L.DpbError("W must be a contiguous fp32 [n, N] tensor on a HIP device")
    n, N = W.shape
    if not (x.is_cuda and x.device == W.device and x.dtype == torch.float32 and x.is_contiguous() and x.numel() == n * N):
        raise L.DpbError(f"x must be a contiguous fp32 tensor of {n * N} elements on {W.device}")
    step = [float(step)] * n if not isinstance(step, (list, tuple)) and not torch.is_tensor(step) else [float(s) for s in step]
    if len(step) != n:
        raise L.DpbError(f"step has {len(step)} entries for {n} rows")
    with torch.cuda.device(W.device):
        st = torch.cuda.current_stream(W.device).cuda_stream
        if out is None:
            out = torch.empty_like(x)
        elif not (out.is_cuda and out.device == W.device and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == n * N):
            raise L.DpbError(f"out must be a contiguous fp32 tensor of {n * N} elements on {W.device}")
        vk = torch.empty_like(W) if return_vk else None
        stats = torch.empty(max(n, 1), 4, dtype=torch.float64, device=W.device)
        need = int(lib.dpb_direction_step_scratch_bytes(n, N))
        scratch = torch.empty(max(need // 8, 1), dtype=torch.float64, device=W.device)
        L.check(lib.dpb_direction_step(_ptr(W), _ptr(x), _ptr(out), _ptr(vk), (C.c_float * max(n, 1))(*step), float(sega_sigma), n, N, _ptr(stats),
                                       _ptr(scratch), need, C.c_void_p(st)))
    return out, vk, stats


def shift_stats(h: torch.Tensor, h0: torch.Tensor, u: torch.Tensor, dirs, signs) -> torch.Tensor:
    """dpb_shift_stats (engine-independent): h, h0 [n, D] and u [nu, D] fp32 on a HIP device, dirs / signs host sequences of n.  Returns [n, 2]
    fp64 on the device: (<h - h0, c> / ||c||, ||h - h0||^2) with c = signs[b] * u[dirs[b]].  No host sync."""
    lib = L.load()
    for name, a in (("h", h), ("h0", h0), ("u", u)):
        if not (a.is_cuda and a.dim() == 2 and a.dtype == torch.float32 and a.is_contiguous()):
            raise L.DpbError(f"{name} must be a contiguous fp32 2-D tensor on a HIP device")
    n, D = h.shape
    if tuple(h0.shape) != (n, D) or u.shape[1] != D:
        raise L.DpbError(f"h {tuple(h.shape)}, h0 {tuple(h0.shape)} and u {tuple(u.shape)} do not agree: [n, D], [n, D], [nu, D]")
    dirs, signs = [int(d) for d in dirs], [float(s) for s in signs]
    if len(dirs) != n or len(signs) != n:
        raise L.DpbError(f"dirs and signs have {len(dirs)} and {len(signs)} entries for {n} rows")
    with torch.cuda.device(h.device):
        st = torch.cuda.current_stream(h.device).cuda_stream
        out = torch.empty(max(n, 1), 2, dtype=torch.float64, device=h.device)
        L.check(lib.dpb_shift_stats(_ptr(h), _ptr(h0), _ptr(u), u.shape[0], (C.c_int32 * max(n, 1))(*dirs), (C.c_float * max(n, 1))(*signs), n, D,
                                    _ptr(out), C.c_void_p(st)))
    return out


def _rows32(name: str, a: torch.Tensor, shape=None, device=None) -> None:
    if not (a.is_cuda and a.dim() == 2 and a.dtype == torch.float32 and a.is_contiguous()) or (device is not None and a.device != device) \
            or (shape is not None and tuple(a.shape) != tuple(shape)):
        raise L.DpbError(f"{name} must be a contiguous fp32 2-D tensor on a HIP device" + (f" of shape {tuple(shape)}" if shape is not None else ""))


class CglsState:
    """The device side of a CGLS solve of R rows (include/dpb.h "The least-squares inverse"): delta, p [R, N] and r [R, D] fp32, updated in place by
    the steps, state [R, 8] fp64 = (gamma, gamma0, mu, ||r||^2, ||delta||^2, flag, ||c||^2, x-steps taken) and the solver's scratch."""

    def __init__(self, R: int, N: int, D: int, device):
        lib = L.load()
        self.R, self.N, self.D = R, N, D
        self.delta = torch.empty(R, N, dtype=torch.float32, device=device)
        self.p = torch.empty(R, N, dtype=torch.float32, device=device)
        self.r = torch.empty(R, D, dtype=torch.float32, device=device)
        self.state = torch.empty(R, 8, dtype=torch.float64, device=device)
        self.need = int(lib.dpb_cgls_init_scratch_bytes(R, N, D))
        self.scratch = torch.empty(max(self.need // 8, 1), dtype=torch.float64, device=device)


def cgls_init(c: torch.Tensor, w0: torch.Tensor, mu_abs: float = 0.0, mu_rel: float = 0.0, tol: float = 0.0, into: Optional[CglsState] = None):
    """dpb_cgls_init (engine-independent): c [R, D] and w0 = J^T c [R, N], fp32 on a HIP device.  Returns (CglsState, hist [R, 4] fp64 = (gamma,
    ||r||^2, ||delta||^2, flag)).  into: a CglsState of the same shape to reuse.  No host sync."""
    lib = L.load()
    _rows32("c", c)
    R, D = c.shape
    _rows32("w0", w0, device=c.device)
    if w0.shape[0] != R:
        raise L.DpbError(f"c has {R} rows, w0 {w0.shape[0]}")
    N = w0.shape[1]
    s = into if into is not None else CglsState(R, N, D, c.device)
    if (s.R, s.N, s.D) != (R, N, D):
        raise L.DpbError(f"the CglsState is for {(s.R, s.N, s.D)}, the call for {(R, N, D)}")
    with torch.cuda.device(c.device):
        st = torch.cuda.current_stream(c.device).cuda_stream
        hist = torch.empty(R, 4, dtype=torch.float64, device=c.device)
        L.check(lib.dpb_cgls_init(_ptr(c), _ptr(w0), _ptr(s.delta), _ptr(s.r), _ptr(s.p), _ptr(s.state), _ptr(hist), float(mu_abs), float(mu_rel),
                                  float(tol), R, N, D, _ptr(s.scratch), s.need, C.c_void_p(st)))
    return s, hist


def cgls_h_step(s: CglsState, q: torch.Tensor) -> torch.Tensor:
    """dpb_cgls_h_step: q = J p [R, D]; updates s.delta and s.r in place and returns the history row [R, 4] fp64.  No host sync."""
    lib = L.load()
    _rows32("q", q, (s.R, s.D), s.delta.device)
    with torch.cuda.device(q.device):
        st = torch.cuda.current_stream(q.device).cuda_stream
        hist = torch.empty(s.R, 4, dtype=torch.float64, device=q.device)
        L.check(lib.dpb_cgls_h_step(_ptr(q), _ptr(s.delta), _ptr(s.r), _ptr(s.p), _ptr(s.state), _ptr(hist), s.R, s.N, s.D, _ptr(s.scratch), s.need,
                                    C.c_void_p(st)))
    return hist


def cgls_x_step(s: CglsState, w: torch.Tensor, tol: float = 0.0) -> torch.Tensor:
    """dpb_cgls_x_step: w = J^T r [R, N]; updates s.p in place and returns the history row [R, 4] fp64.  No host sync."""
    lib = L.load()
    _rows32("w", w, (s.R, s.N), s.delta.device)
    with torch.cuda.device(w.device):
        st = torch.cuda.current_stream(w.device).cuda_stream
        hist = torch.empty(s.R, 4, dtype=torch.float64, device=w.device)
        L.check(lib.dpb_cgls_x_step(_ptr(w), _ptr(s.delta), _ptr(s.r), _ptr(s.p), _ptr(s.state), _ptr(hist), float(tol), s.R, s.N, s.D,
                                    _ptr(s.scratch), s.need, C.c_void_p(st)))
    return hist


def newton_residual(h0: torch.Tensor, h: torch.Tensor, u: torch.Tensor, dirs, signs, scale, frac: float) -> torch.Tensor:
    """dpb_newton_residual (engine-independent): res[b] = h0[b] + frac * scale[b] * signs[b] * u[dirs[b]] - h[b], formed in fp64 and rounded once;
    h0, h [n, D] and u [nu, D] fp32 on a HIP device, dirs / signs / scale host sequences of n.  No host sync."""
    lib = L.load()
    _rows32("h0", h0)
    n, D = h0.shape
    _rows32("h", h, (n, D), h0.device)
    _rows32("u", u, device=h0.device)
    if u.shape[1] != D:
        raise L.DpbError(f"u {tuple(u.shape)} does not hold directions of {D} elements")
    dirs, signs, scale = [int(d) for d in dirs], [float(s) for s in signs], [float(s) for s in scale]
    if not (len(dirs) == len(signs) == len(scale) == n):
        raise L.DpbError(f"dirs, signs and scale have {len(dirs)}, {len(signs)} and {len(scale)} entries for {n} rows")
    with torch.cuda.device(h0.device):
        st = torch.cuda.current_stream(h0.device).cuda_stream
        res = torch.empty_like(h0)
        L.check(lib.dpb_newton_residual(_ptr(h0), _ptr(h), _ptr(u), u.shape[0], (C.c_int32 * n)(*dirs), (C.c_float * n)(*signs), (C.c_float * n)(*scale),
                                        float(frac), n, D, _ptr(res), C.c_void_p(st)))
    return res


def newton_update(x: torch.Tensor, delta: torch.Tensor, state: torch.Tensor, radius: float = 0.0):
    """dpb_newton_update (engine-independent): x_out[b] = x[b] + kappa_b * delta[b], kappa_b = min(1, radius / ||delta_b||) (radius = 0: no clamp) with
    ||delta_b||^2 from the solver's state [n, 8] fp64.  Returns (x_out, step_stats [n, 4] fp64 = (||res||^2, ||delta||^2, kappa, flag)).  No host sync."""
    lib = L.load()
    _rows32("x", x)
    n, N = x.shape
    _rows32("delta", delta, (n, N), x.device)
    if not (state.is_cuda and state.device == x.device and state.dtype == torch.float64 and state.is_contiguous() and tuple(state.shape) == (n, 8)):
        raise L.DpbError(f"state must be a contiguous fp64 [{n}, 8] tensor on {x.device}")
    with torch.cuda.device(x.device):
        st = torch.cuda.current_stream(x.device).cuda_stream
        out = torch.empty_like(x)
        stats = torch.empty(n, 4, dtype=torch.float64, device=x.device)
        L.check(lib.dpb_newton_update(_ptr(x), _ptr(delta), _ptr(state), float(radius), _ptr(out), _ptr(stats), n, N, C.c_void_p(st)))
    return out, stats


def _curve_rows(name: str, a: torch.Tensor, rows: Optional[int] = None, device=None) -> None:
    if not (a.is_cuda and a.dim() == 2 and a.dtype == torch.float32 and a.is_contiguous()):
        raise L.DpbError(f"{name} must be a contiguous fp32 2-D tensor on a HIP device")
    if rows is not None and (a.shape[0] != rows or a.device != device):
        raise L.DpbError(f"{name} has {a.shape[0]} rows on {a.device}, expected {rows} on {device}")


def geodesic_cotangents(h: torch.Tensor, cot: Optional[torch.Tensor] = None, return_csq: bool = True):
    """dpb_geodesic_cotangents (engine-independent): h [m + 2, D] fp32 on a HIP device, the tap activations along a curve.  Returns (cot [m, D] fp32 =
    2 h_i - h_{i-1} - h_{i+1} formed in fp64 and rounded once, seg [m + 1] fp64 = ||h_{i+1} - h_i||^2, csq [m] fp64 = ||cot_i||^2 or None).  cot: the
    tensor written into, allocated here when None.  No host sync (include/dpb.h states the arithmetic)."""
    lib = L.load()
    _curve_rows("h", h)
    n, D = h.shape
    m = n - 2
    with torch.cuda.device(h.device):
        st = torch.cuda.current_stream(h.device).cuda_stream
        if cot is None:
            cot = torch.empty(max(m, 1), D, dtype=torch.float32, device=h.device)
        else:
            _curve_rows("cot", cot, max(m, 1), h.device)
        seg = torch.empty(max(m, 1) + 1, dtype=torch.float64, device=h.device)
        csq = torch.empty(max(m, 1), dtype=torch.float64, device=h.device) if return_csq else None
        need = int(lib.dpb_geodesic_cotangents_scratch_bytes(m, D))
        scratch = torch.empty(max(need // 8, 1), dtype=torch.float64, device=h.device)
        L.check(lib.dpb_geodesic_cotangents(_ptr(h), _ptr(cot), _ptr(seg), _ptr(csq), m, D, _ptr(scratch), need, C.c_void_p(st)))
    return cot, seg, csq


def geodesic_update(P: torch.Tensor, W: torch.Tensor, eta: float, lam: float = 0.0, out: Optional[torch.Tensor] = None):
    """dpb_geodesic_update (engine-independent): P [m + 2, N] (a curve) and W [m, N] (the adjoint results J^T c of its interior rows), fp32 on a HIP
    device.  Returns (P_out [m + 2, N] with P_out_i = P_i - eta (W_i + lam (2 P_i - P_{i-1} - P_{i+1})) for the interior rows and the end rows
    copied, stats [m, 4] fp64 = (||W_i||^2, ||g_i||^2, ||P_out_i - P_i||^2, flag), xseg [m + 1] fp64 = ||P_{i+1} - P_i||^2 of P).  out: the tensor
    written into -- it must not overlap P -- allocated here when None.  A row that meets a non-finite value has its flag set and NaN in its row of
    P_out.  No host sync."""
    lib = L.load()
    _curve_rows("P", P)
    n, N = P.shape
    m = n - 2
    _curve_rows("W", W, max(m, 1), P.device)
    if W.shape[1] != N:
        raise L.DpbError(f"W {tuple(W.shape)} and P {tuple(P.shape)} do not agree: [m, N] and [m + 2, N]")
    with torch.cuda.device(P.device):
        st = torch.cuda.current_stream(P.device).cuda_stream
        if out is None:
            out = torch.empty_like(P)
        else:
            _curve_rows("out", out, n, P.device)
            if out.shape[1] != N:
                raise L.DpbError(f"out {tuple(out.shape)} and P {tuple(P.shape)} do not agree")
        stats = torch.empty(max(m, 1), 4, dtype=torch.float64, device=P.device)
        xseg = torch.empty(max(m, 1) + 1, dtype=torch.float64, device=P.device)
        need = int(lib.dpb_geodesic_update_scratch_bytes(m, N))
        scratch = torch.empty(max(need // 8, 1), dtype=torch.float64, device=P.device)
        L.check(lib.dpb_geodesic_update(_ptr(P), _ptr(W), _ptr(out), float(eta), float(lam), m, N, _ptr(stats), _ptr(xseg), _ptr(scratch), need,
                                        C.c_void_p(st)))
    return out, stats, xseg


def ddim_step_asym(x: torch.Tensor, e: torch.Tensor, e_s: torch.Tensor, alpha_t: float, alpha_next: float, gP: float = 1.0, gD: float = 0.0,
                   out: Optional[torch.Tensor] = None, return_x0: bool = True):
    """dpb_ddim_step_asym (engine-independent): per row of x, e, e_s [n, N] (fp32 on a HIP device) the asymmetric DDIM step d = e_s - e,
    eP = e + gP d, eD = e + gD d, P = (x - eP sqrt(1 - alpha_t)) / sqrt(alpha_t), out = sqrt(alpha_next) P + sqrt(1 - alpha_next) eD, fp32 in
    dpb_ddim_step's operation order.  out: the tensor written into (x itself for an in-place step), allocated here when None.  Returns (out, P or
    None, stats [n, 2] fp64 = (sum d^2, flag)); a row holding a non-finite value has its flag set and NaN in its row of out and P.  No host sync."""
    lib = L.load()
    if not (x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and x.is_contiguous()):
        raise L.DpbError("x must be a contiguous fp32 [n, N] tensor on a HIP device")
    n, N = x.shape
    for name, a in (("e", e), ("e_s", e_s)):
        if not (a.is_cuda and a.device == x.device and a.dtype == torch.float32 and a.is_contiguous() and a.numel() == n * N):
            raise L.DpbError(f"{name} must be a contiguous fp32 tensor of {n * N} elements on {x.device}")
    with torch.cuda.device(x.device):
        st = torch.cuda.current_stream(x.device).cuda_stream
        if out is None:
            out = torch.empty_like(x)
        elif not (out.is_cuda and out.device == x.device and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == n * N):
            raise L.DpbError(f"out must be a contiguous fp32 tensor of {n * N} elements on {x.device}")
        x0 = torch.empty_like(x) if return_x0 else None
        stats = torch.empty(max(n, 1), 2, dtype=torch.float64, device=x.device)
        need = int(lib.dpb_ddim_step_asym_scratch_bytes(n, N))
        scratch = torch.empty(max(need // 8, 1), dtype=torch.float64, device=x.device)
        L.check(lib.dpb_ddim_step_asym(_ptr(x), _ptr(e), _ptr(e_s), _ptr(out), _ptr(x0), n, N, float(alpha_t), float(alpha_next), float(gP), float(gD),
                                       _ptr(stats), _ptr(scratch), need, C.c_void_p(st)))
    return out, x0, stats
