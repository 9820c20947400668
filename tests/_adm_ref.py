"""CPU restatement of the guided-diffusion (ADM) U-Net forward: functional, on a params dict with the reference's state-dict names.

Test infrastructure (not imported by the product).  Written from the reference's module tree (src/models/guided_diffusion/unet.py:162-258
ResBlock, :261-391 attention, :398-702 UNetModel) and pinned to the reference's own outputs by tests/test_adm_host.py (fixtures of
tests/golden/make_golden_adm.py).  ``forward(p, cfg, x, t, stop=)`` stops at a tap; ``get_h_to_e(p, cfg, x, t, h)`` continues from the middle
block's output with every skip taken from x.  Works in the dtype of the parameters (fp32 for the pins, fp64 for the Jacobian references) and is
differentiable (torch.func.jvp / vjp, autograd).
"""
import math

import torch
import torch.nn.functional as F

from diffusion_pullback_amd.configs import ADMConfig, adm_blocks

# the toy configurations of the ADM tests: the smallest at which each new piece can go wrong
T1 = ADMConfig(image_size=16, model_channels=32, channel_mult=(1, 2), num_res_blocks=1, attention_resolutions=(8,), num_head_channels=16,
               use_scale_shift_norm=True, resblock_updown=True, use_new_attention_order=False, learn_sigma=True)
T2 = ADMConfig(image_size=32, model_channels=64, channel_mult=(1, 2), num_res_blocks=1, attention_resolutions=(16,), num_head_channels=64,
               use_scale_shift_norm=True, resblock_updown=True, use_new_attention_order=True, learn_sigma=True)
T3 = ADMConfig(image_size=16, model_channels=32, channel_mult=(1, 2), num_res_blocks=1, attention_resolutions=(8,), num_head_channels=16,
               use_scale_shift_norm=False, resblock_updown=False, use_new_attention_order=False, learn_sigma=True)
TOYS = {"T1": T1, "T2": T2, "T3": T3}
# Their synthetic weights, configs.adm_init_params(cfg, **init_kwargs(TOY_INIT[name])), and the seed their inputs are drawn under.  T1 carries the
# pullback pin: a plain random toy net has a flat spectrum (sigma_2 / sigma_1 = 0.94, sigma_5 / sigma_4 = 0.997 at seed 0), so its middle
# attention is shaped (configs.Spectrum) -- fp64 full-Jacobian singular values 42.4, 33.5, 20.1, 16.2, 14.8: the top four separated by 9 % or more.
TOY_INIT = {"T1": dict(seed=0, gain=1.0, spectrum=dict(rank=6, decay=0.7, amp=40.0), input_seed=5),
            "T2": dict(seed=1, gain=1.0, spectrum=None, input_seed=6),
            "T3": dict(seed=2, gain=1.0, spectrum=None, input_seed=7)}


def init_kwargs(init):
    from diffusion_pullback_amd.configs import Spectrum
    return dict(seed=init["seed"], gain=init["gain"], spectrum=Spectrum(**init["spectrum"]) if init["spectrum"] else None)


def timestep_embedding(t, dim):
    half = dim // 2
    freqs = torch.exp(-math.log(10000) * torch.arange(half, dtype=torch.float32) / half)
    args = t[:, None].float() * freqs[None]
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1)


def _gn(p, n, x, cfg):
    return F.group_norm(x, cfg.groups, p[n + ".weight"], p[n + ".bias"], cfg.gn_eps)


def _conv(p, n, x, **kw):
    return F.conv2d(x, p[n + ".weight"], p[n + ".bias"], **kw)


def _resblock(p, cfg, n, x, emb, kind):
    h = F.silu(_gn(p, n + ".in_layers.0", x, cfg))
    if kind == "res_down":
        h, x = F.avg_pool2d(h, 2), F.avg_pool2d(x, 2)
    elif kind == "res_up":
        h, x = F.interpolate(h, scale_factor=2, mode="nearest"), F.interpolate(x, scale_factor=2, mode="nearest")
    h = _conv(p, n + ".in_layers.2", h, padding=1)
    e = F.linear(F.silu(emb), p[n + ".emb_layers.1.weight"], p[n + ".emb_layers.1.bias"])[:, :, None, None]
    if cfg.use_scale_shift_norm:
        scale, shift = e.chunk(2, dim=1)
        h = _gn(p, n + ".out_layers.0", h, cfg) * (1 + scale) + shift
    else:
        h = _gn(p, n + ".out_layers.0", h + e, cfg)
    h = _conv(p, n + ".out_layers.3", F.silu(h), padding=1)
    if n + ".skip_connection.weight" in p:
        x = _conv(p, n + ".skip_connection", x)
    return x + h


def _attn(p, cfg, n, x):
    b, c, hh, ww = x.shape
    heads = cfg.heads_for(c)
    d = c // heads
    xf = x.reshape(b, c, -1)
    qkv = F.conv1d(_gn(p, n + ".norm", xf, cfg), p[n + ".qkv.weight"], p[n + ".qkv.bias"])
    L = qkv.shape[-1]
    if cfg.use_new_attention_order:
        q, k, v = (a.reshape(b * heads, d, L) for a in qkv.chunk(3, dim=1))
    else:
        q, k, v = qkv.reshape(b * heads, 3 * d, L).split(d, dim=1)
    w = torch.softmax(torch.einsum("bct,bcs->bts", q, k) / math.sqrt(d), dim=-1)
    a = torch.einsum("bts,bcs->bct", w, v).reshape(b, c, L)
    return (xf + F.conv1d(a, p[n + ".proj_out.weight"], p[n + ".proj_out.bias"])).reshape(b, c, hh, ww)


def _emb(p, cfg, t, b, dtype):
    t = torch.as_tensor(t, dtype=torch.float32).reshape(-1)
    e = timestep_embedding(t, cfg.model_channels).to(dtype)
    e = F.linear(e, p["time_embed.0.weight"], p["time_embed.0.bias"])
    e = F.linear(F.silu(e), p["time_embed.2.weight"], p["time_embed.2.bias"])
    return e.expand(b, -1) if e.shape[0] == 1 else e


def _encoder(p, cfg, x, emb, blocks):
    hs, h = [], x
    for name, kind, cin, cout, ds in blocks:
        if name.startswith("middle_block"):
            break
        if kind == "conv_in":
            h = _conv(p, name, h, padding=1)
        elif kind == "attn":
            h = _attn(p, cfg, name, h)
            hs.pop()
        elif kind == "down":
            h = _conv(p, name + ".op", h, stride=2, padding=1)
        else:
            h = _resblock(p, cfg, name, h, emb, kind)
        hs.append(h)
    h = _resblock(p, cfg, "middle_block.0", h, emb, "res")
    h = _attn(p, cfg, "middle_block.1", h)
    h = _resblock(p, cfg, "middle_block.2", h, emb, "res")
    return h, hs


def _decoder(p, cfg, h, hs, emb, blocks):
    hs = list(hs)
    for name, kind, cin, cout, ds in blocks:
        if not name.startswith("output_blocks"):
            continue
        if kind == "res":
            h = _resblock(p, cfg, name, torch.cat([h, hs.pop()], dim=1), emb, kind)
        elif kind == "attn":
            h = _attn(p, cfg, name, h)
        elif kind == "up":
            h = _conv(p, name + ".conv", F.interpolate(h, scale_factor=2, mode="nearest"), padding=1)
        else:
            h = _resblock(p, cfg, name, h, emb, kind)
    h = _conv(p, "out.2", F.silu(_gn(p, "out.0", h, cfg)), padding=1)
    return h[:, :cfg.in_channels] if cfg.learn_sigma else h      # UNetModel.forward returns et (unet.py:680-684)


def forward(p, cfg, x, t, stop=None):
    """eps [B, 3, S, S] (stop=None / 'eps') or the middle block's output (stop=('mid', 0)); t: one timestep or one per sample"""
    blocks = adm_blocks(cfg)
    emb = _emb(p, cfg, t, x.shape[0], x.dtype)
    h, hs = _encoder(p, cfg, x, emb, blocks)
    if stop == ("mid", 0):
        return h
    assert stop in (None, "eps"), stop
    return _decoder(p, cfg, h, hs, emb, blocks)


def get_h(p, cfg, x, t):
    return forward(p, cfg, x, t, stop=("mid", 0))


def get_h_to_e(p, cfg, x, t, h):
    """eps with the middle block's output replaced by h [B, C, H, W]; the skips are those of the single sample x, repeated"""
    blocks = adm_blocks(cfg)
    b = h.shape[0]
    emb = _emb(p, cfg, t, x.shape[0], x.dtype)
    _, hs = _encoder(p, cfg, x, emb, blocks)
    rep = lambda a: a.expand(b, *a.shape[1:]) if a.shape[0] == 1 and b > 1 else a
    return _decoder(p, cfg, h, [rep(a) for a in hs], rep(emb), blocks)


def to_dtype(p, dtype):
    return {k: v.to(dtype) for k, v in p.items()}


def full_jacobian_svd(f, cfg, dtype=torch.float64):
    """(singular values, Vh) of d get_h / d x at the fixture's (x, t), from the restatement's full Jacobian in `dtype`"""
    from diffusion_pullback_amd.configs import adm_init_params
    p = to_dtype(adm_init_params(cfg, **init_kwargs(f["init"])), dtype)
    x = f["x"].to(dtype)
    J = torch.func.jacfwd(lambda a: get_h(p, cfg, a, f["t"]).reshape(-1))(x).reshape(-1, x.numel())
    _, s, Vh = torch.linalg.svd(J, full_matrices=False)
    return s, Vh


def separated(sv, k, gap=0.05):
    """for each of the top k singular values: is it more than `gap` (relative) away from both neighbours?"""
    out = []
    for i in range(k):
        up = i == 0 or sv[i] < (1 - gap) * sv[i - 1]
        dn = sv[i + 1] < (1 - gap) * sv[i]
        out.append(bool(up and dn))
    return out
