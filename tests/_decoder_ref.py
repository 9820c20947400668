"""CPU restatement of get_h_to_e -- the U-Net from a tap on, every skip connection held at its primal value -- for the decoder
pullback tests, built from oracle/'s functional blocks (fp32, autodiff-able in input_h).

Semantics (reference: PullBackDDPM.get_h_to_e, src/models/ddpm/diffusion.py:273-345; utils.get_h_to_e, src/utils/utils.py:529-635):
the forward runs at the single sample x up to the tap (op, idx), the activation there is replaced by input_h [B, C, H, W], the skips,
time embedding and text context are repeated B times, and the forward continues to eps.  A 'down' tap is the block output after its
downsampler, which is also the last skip of that block: both are replaced (utils.py:575-579).  The reference's own DDPM code asserts
op == 'mid' and its SD code takes 'mid' / 'down'; this restatement covers every tap the engine accepts.
"""
import torch
import torch.nn.functional as F

from oracle import unet_ddpm as od
from oracle import unet_sd as osd


def _rep(a, b):
    return a.expand(b, *a.shape[1:])


def sd_h_to_e(p, cfg, x, t, ctx, input_h, op, idx):
    """x [1, C, H, W], ctx [1, L, D] -> eps [B, C, H, W] with the activation at (op, idx) replaced by input_h [B, ...]"""
    osd.check_params(p, cfg)
    b = input_h.shape[0]
    if not torch.is_tensor(t):
        t = torch.tensor([float(t)])
    t = t.reshape(-1)[:1]
    emb = osd.timestep_embedding(t, cfg.block_out_channels[0]).to(x.dtype)
    emb = osd._lin(p, "time_embedding.linear_2", F.silu(osd._lin(p, "time_embedding.linear_1", emb)))
    stop = (op, idx)
    seeded = []

    def seed(skips):
        seeded.append(stop)
        return input_h, [_rep(s, b) for s in skips], _rep(emb, b), _rep(ctx, b)

    h = osd._conv(p, "conv_in", x)
    skips = [h]
    nb = len(cfg.block_out_channels)
    for i in range(nb):
        for j in range(cfg.layers_per_block):
            h = osd._resnet(p, f"down_blocks.{i}.resnets.{j}", h, emb, cfg)
            if cfg.down_attn[i]:
                h = osd._transformer(p, f"down_blocks.{i}.attentions.{j}", h, ctx, cfg.heads[i], cfg)
            skips.append(h)
        if i != nb - 1:
            h = osd._conv(p, f"down_blocks.{i}.downsamplers.0.conv", h, stride=2, padding=1)
            skips.append(h)
        if stop == ("down", i):
            h, skips, emb, ctx = seed(skips)
            skips[-1] = input_h
    h = osd._resnet(p, "mid_block.resnets.0", h, emb, cfg)
    h = osd._transformer(p, "mid_block.attentions.0", h, ctx, cfg.heads[-1], cfg)
    h = osd._resnet(p, "mid_block.resnets.1", h, emb, cfg)
    if stop == ("mid", 0):
        h, skips, emb, ctx = seed(skips)
    rheads = tuple(reversed(cfg.heads))
    for i in range(nb):
        for j in range(cfg.layers_per_block + 1):
            h = osd._resnet(p, f"up_blocks.{i}.resnets.{j}", torch.cat([h, skips.pop()], dim=1), emb, cfg)
            if cfg.up_attn[i]:
                h = osd._transformer(p, f"up_blocks.{i}.attentions.{j}", h, ctx, rheads[i], cfg)
        if i != nb - 1:
            h = osd._conv(p, f"up_blocks.{i}.upsamplers.0.conv", F.interpolate(h, scale_factor=2.0, mode="nearest"))
        if stop == ("up", i):
            h, skips, emb, ctx = seed(skips)
    if not seeded:
        raise ValueError(f"(op, block_idx) = {stop} is not valid")
    return osd._conv(p, "conv_out", F.silu(osd._gn(p, "conv_norm_out", h, cfg.groups, 1e-5)))


def ddpm_h_to_e(p, cfg, x, t, input_h, op, idx):
    """x [1, C, H, W] -> eps [B, C, H, W] with the activation at (op, idx) replaced by input_h [B, ...]"""
    b = input_h.shape[0]
    if not torch.is_tensor(t):
        t = torch.tensor([t])
    t = t.reshape(-1)[:1]
    temb = od.timestep_embedding(t, cfg.ch)
    temb = F.linear(temb, p["temb.dense.0.weight"], p["temb.dense.0.bias"])
    temb = F.linear(od._swish(temb), p["temb.dense.1.weight"], p["temb.dense.1.bias"])
    stop = (op, idx)
    seeded = False
    nres = len(cfg.ch_mult)
    res = cfg.resolution
    hs = [od._conv(p, "conv_in", x)]
    for lvl in range(nres):
        for blk in range(cfg.num_res_blocks):
            h = od._resblock(p, f"down.{lvl}.block.{blk}", hs[-1], temb, cfg)
            if res in cfg.attn_resolutions:
                h = od._attn(p, f"down.{lvl}.attn.{blk}", h, cfg)
            hs.append(h)
        if lvl != nres - 1:
            hs.append(od._down(p, f"down.{lvl}.downsample", hs[-1]))
            res //= 2
        if stop == ("down", lvl):
            hs = [_rep(s, b) for s in hs[:-1]] + [input_h]
            temb, seeded = _rep(temb, b), True
    h = od._resblock(p, "mid.block_1", hs[-1], temb, cfg)
    h = od._attn(p, "mid.attn_1", h, cfg)
    h = od._resblock(p, "mid.block_2", h, temb, cfg)
    if stop == ("mid", 0):
        h, hs, temb, seeded = input_h, [_rep(s, b) for s in hs], _rep(temb, b), True
    for lvl in reversed(range(nres)):
        for blk in range(cfg.num_res_blocks + 1):
            h = od._resblock(p, f"up.{lvl}.block.{blk}", torch.cat([h, hs.pop()], dim=1), temb, cfg)
            if res in cfg.attn_resolutions:
                h = od._attn(p, f"up.{lvl}.attn.{blk}", h, cfg)
        if lvl != 0:
            h = od._up(p, f"up.{lvl}.upsample", h)
            res *= 2
        if stop == ("up", lvl):
            h, hs, temb, seeded = input_h, [_rep(s, b) for s in hs], _rep(temb, b), True
    if not seeded:
        raise ValueError(f"(op, block_idx) = {stop} is not valid")
    return od._conv(p, "conv_out", od._swish(od._gn(p, "norm_out", h, cfg)))


def power_loop(f, h0, V0, n_iters):
    """n_iters plain power iterations of J = df/dh at h0 (fp32 CPU, one row at a time): V <- rows of svd(J^T J V), U = J V_prev of the
    last iteration.  Returns (V [k, N_h], s = sqrt(singular values of J^T J V_prev) [k], U [k, N_out]) -- the decoder's (u^T, s, vT)."""
    V = V0.clone()
    for _ in range(n_iters):
        U = torch.stack([torch.func.jvp(f, (h0,), (v.reshape(h0.shape),))[1].reshape(-1) for v in V])
        hh = h0.clone().requires_grad_(True)
        out = f(hh)
        W = torch.stack([torch.autograd.grad(out, hh, u.reshape(out.shape), retain_graph=True)[0].reshape(-1) for u in U])
        _, s, V = torch.linalg.svd(W, full_matrices=False)
    return V, s.sqrt(), U
