"""The h-space guidance edit restated in float64 / float32 torch on the oracle's CPU nets.

A chain carries a state x, a direction c at the tap and a scale s; step j over (t, a, a_next):
    e = eps(x, t),  e_s = eps(x, t | h <- h + s c),  d = e_s - e,  eP = e + gP d,  eD = e + gD d,
    P = (x - eP sqrt(1 - a)) / sqrt(a),  x' = sqrt(a_next) P + sqrt(1 - a_next) eD.
e is the oracle's forward, e_s the tap-to-eps restatement of tests/_decoder_ref.py (tests/_adm_ref.py for ADM) at h + s c, h the oracle's get_h."""
import torch

import _adm_ref as A
from _decoder_ref import ddpm_h_to_e, sd_h_to_e


def step_ref(x, e, es, a, an, gP, gD):
    """one step in the dtype of x (the alphas are cast to it first, their square roots taken in it); returns (x', P, d)"""
    a, an = torch.as_tensor(a, dtype=x.dtype), torch.as_tensor(an, dtype=x.dtype)
    d = es - e
    eP, eD = e + gP * d, e + gD * d
    P = (x - eP * (1 - a).sqrt()) / a.sqrt()
    return an.sqrt() * P + (1 - an).sqrt() * eD, P, d


def dx_coef(a, an, gP, gD):
    """x' - x'_plain = coef * d, the plain step being that of e alone"""
    a, an = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(an, dtype=torch.float64)
    return -an.sqrt() * (1 - a).sqrt() / a.sqrt() * gP + (1 - an).sqrt() * gD


def nets(kind, cfg, p, ctx, tap, dtype):
    """(eps(x [n], t), eps_shifted(x [n], t, shift [n, N_h])) with parameters in `dtype`; ctx [n, L, D] or None (row b belongs to sample b)"""
    p = {k: v.to(dtype) for k, v in p.items()}
    if kind == "sd":
        from oracle import unet_sd

        def eps(x, t):
            return unet_sd.forward(p, cfg, x, torch.tensor(t), ctx.to(dtype))

        def eps_s(x, t, shift):
            out = []
            for b in range(x.shape[0]):
                h = unet_sd.forward(p, cfg, x[b:b + 1], torch.tensor(t), ctx[b:b + 1].to(dtype), stop=tap)
                out.append(sd_h_to_e(p, cfg, x[b:b + 1], torch.tensor(t), ctx[b:b + 1].to(dtype), h + shift[b].reshape(h.shape), *tap))
            return torch.cat(out)
        return eps, eps_s
    if kind == "ddpm":
        from oracle import unet_ddpm
        emb = unet_ddpm.timestep_embedding

        def cast(f):                                              # the oracle's sinusoid is fp32 whatever the parameters: cast it for the float64 run
            def g(*a):
                unet_ddpm.timestep_embedding = lambda t, d: emb(t, d).to(dtype)
                try:
                    return f(*a)
                finally:
                    unet_ddpm.timestep_embedding = emb
            return g

        @cast
        def eps(x, t):
            return unet_ddpm.forward(p, cfg, x, torch.tensor(t))

        @cast
        def eps_s(x, t, shift):
            out = []
            for b in range(x.shape[0]):
                h = unet_ddpm.forward(p, cfg, x[b:b + 1], torch.tensor(t), stop=tap)
                out.append(ddpm_h_to_e(p, cfg, x[b:b + 1], torch.tensor(t), h + shift[b].reshape(h.shape), *tap))
            return torch.cat(out)
        return eps, eps_s
    assert kind == "adm" and tap == ("mid", 0), "tests/_adm_ref.py restates the middle block's tap only"

    def eps(x, t):
        return A.forward(p, cfg, x, t)

    def eps_s(x, t, shift):
        out = []
        for b in range(x.shape[0]):
            h = A.get_h(p, cfg, x[b:b + 1], t)
            out.append(A.get_h_to_e(p, cfg, x[b:b + 1], t, h + shift[b].reshape(h.shape)))
        return torch.cat(out)
    return eps, eps_s


def chain_ref(net, x, c, scales, ts, alphas, alphas_next, gP, gD, dtype=torch.float64):
    """net = nets(...); x [n, ...]; c [n, N_h] unit directions; scales [n]; returns states [n, S + 1, ...], delta_norm [n, S], dx_norm [n, S]"""
    eps, eps_s = net
    x = x.to(dtype)
    shift = (torch.as_tensor(scales, dtype=torch.float64)[:, None] * c.double()).to(dtype)
    states, dn, dxn = [x], [], []
    with torch.no_grad():
        for t, a, an in zip(ts, alphas, alphas_next):
            e, es = eps(x, t), eps_s(x, t, shift)
            x, _, d = step_ref(x, e, es, a, an, gP, gD)
            states.append(x)
            dn.append(d.double().flatten(1).norm(dim=1))
            dxn.append(dn[-1] * float(dx_coef(a, an, gP, gD).abs()))
    return {"states": torch.stack(states, dim=1), "delta_norm": torch.stack(dn, dim=1), "dx_norm": torch.stack(dxn, dim=1)}


def resync_ref(net, ref64, c, scales, ts, alphas, alphas_next, gP, gD, dtype):
    """the one-step restatement: step j started from the float64 chain's state j, in `dtype`; the same keys, states [n, S, ...] the results"""
    out = {"states": [], "delta_norm": [], "dx_norm": []}
    for j in range(len(ts)):
        r = chain_ref(net, ref64["states"][:, j].float(), c, scales, ts[j:j + 1], alphas[j:j + 1], alphas_next[j:j + 1], gP, gD, dtype)
        out["states"].append(r["states"][:, 1]); out["delta_norm"].append(r["delta_norm"][:, 0]); out["dx_norm"].append(r["dx_norm"][:, 0])
    return {k: torch.stack(v, dim=1) for k, v in out.items()}
