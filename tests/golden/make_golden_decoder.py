"""Generate the decoder-pullback golden fixtures by IMPORTING THE REFERENCE (same recipe as make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_decoder.py

Fixtures (tensors only)
  decoder_xt_ddpm.pt   PullBackDDPM.local_decoder_pullback_xt / local_x0_decoder_pullback_xt (diffusion.py:558-632, :634-710) of the
                       reduced-width vendored DDPM of ddpm_small.pt (weights = oracle.unet_ddpm.init_params(cfg, seed)), op = 'mid'
  decoder_zt_tiny.pt   utils.local_decoder_pullback_zt (utils.py:818-898) bound onto the toy SD net of pullback_zt_tiny.pt, whose
                       get_h / get_h_to_e are oracle.unet_sd's forward and tests/_decoder_ref.py's restatement ('mid', 'down', 'up' taps)
Every case records the RNG seed the reference draws its start basis from, that basis (V0 = Q^T), the loop parameters, the returned
(u, s, vT) and the number of iterations the reference ran (counted from its per-iteration print).
"""
import contextlib
import io
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from make_golden import import_reference   # noqa: E402


def _run(fn, rng_seed):
    """fn() after seeding the global RNG the reference draws its start basis from; returns (result, iterations it ran)"""
    import torch
    torch.manual_seed(rng_seed)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = fn()
    iters = sum(1 for line in buf.getvalue().splitlines() if "-th step convergence" in line)
    return out, iters


def _v0(n, k, rng_seed):
    import torch
    torch.manual_seed(rng_seed)
    q, _ = torch.linalg.qr(torch.randn(n, k))                 # diffusion.py:585-588, utils.py:843-846
    return q.T.contiguous()


def main():
    import torch
    torch.set_num_threads(8)
    ru, rd = import_reference()
    from oracle import unet_ddpm, unet_sd
    from _decoder_ref import ddpm_h_to_e, sd_h_to_e

    # ---------------------------------------------------------------- vendored DDPM, reduced width (ddpm_small.pt's net and inputs)
    small = torch.load(os.path.join(HERE, "ddpm_small.pt"), weights_only=False)
    cfgd = small["cfg"]
    cfg = unet_ddpm.DDPMConfig(**cfgd)
    ns = ru.dict2namespace({"config": {"model": dict(ch=cfgd["ch"], out_ch=cfgd["out_ch"], ch_mult=list(cfgd["ch_mult"]),
                                                   num_res_blocks=cfgd["num_res_blocks"], attn_resolutions=list(cfgd["attn_resolutions"]),
                                                   dropout=0.0, in_channels=cfgd["in_channels"], resamp_with_conv=True),
                                      "data": dict(image_size=cfgd["resolution"])}})
    ns.device = "cpu"; ns.dtype = torch.float32
    net = rd.PullBackDDPM(ns).eval()
    params = unet_ddpm.init_params(cfg, seed=small["seed"])
    net.load_state_dict(params, strict=True)
    x, t = small["x"], small["t"]
    with torch.no_grad():                                      # the restatement is the vendored get_h_to_e at 'mid'
        h = net.get_h(x, t, op="mid", block_idx=0)
        hb = h + 0.1 * torch.randn(2, *h.shape[1:], generator=torch.Generator().manual_seed(1))
        e_ref = net.get_h_to_e(x=x, t=t, input_h=hb, op="mid", block_idx=0)
        e_re = ddpm_h_to_e(params, cfg, x, t, hb, "mid", 0)
        assert (e_ref - e_re).norm() / e_ref.norm() < 1e-5, "restatement disagrees with PullBackDDPM.get_h_to_e"
    n_h = h.numel()
    fix = {"cfg": cfgd, "seed": small["seed"], "x": x, "t": t, "at": torch.tensor(0.6), "xt": [], "x0": []}
    # (k, chunk_size, min_iter, max_iter, thr, rng_seed): the first stops early, the second runs to max_iter.  The reference's stop test is
    # allclose(v_prev, v, atol=thr) on LAPACK's arbitrary singular-vector signs, which flip between iterations here; with thr = 0.5 (every
    # |v_i| < 0.25) it fires whatever the signs, at the first i > min_iter -- as the product's sign-aligned rule does: the iteration counts agree.
    for (k, chunk, mn, mx, thr, rs) in [(3, 2, 3, 30, 0.5, 31), (2, 2, 1, 4, 1e-9, 32)]:
        (u, s, vT), it = _run(lambda: net.local_decoder_pullback_xt(x=x, t=t, op="mid", block_idx=0, pca_rank=k, chunk_size=chunk,
                                                                    min_iter=mn, max_iter=mx, convergence_threshold=thr), rs)
        fix["xt"].append(dict(k=k, chunk_size=chunk, min_iter=mn, max_iter=mx, thr=thr, rng_seed=rs, V0=_v0(n_h, k, rs), iters=it,
                              u=u.clone(), s=s.clone(), vT=vT.clone()))
        print("decoder_xt", k, it)
    for (k, chunk, mn, mx, thr, rs) in [(3, 1, 3, 30, 0.5, 33), (2, 2, 1, 3, 1e-9, 34)]:
        (u, s, vT), it = _run(lambda: net.local_x0_decoder_pullback_xt(x=x, t=t, at=fix["at"], op="mid", block_idx=0, pca_rank=k,
                                                                       chunk_size=chunk, min_iter=mn, max_iter=mx, convergence_threshold=thr), rs)
        fix["x0"].append(dict(k=k, chunk_size=chunk, min_iter=mn, max_iter=mx, thr=thr, rng_seed=rs, V0=_v0(n_h, k, rs), iters=it,
                              u=u.clone(), s=s.clone(), vT=vT.clone()))
        print("decoder_x0", k, it)
    torch.save(fix, os.path.join(HERE, "decoder_xt_ddpm.pt"))

    # ---------------------------------------------------------------- utils.local_decoder_pullback_zt on the toy SD net
    tiny = torch.load(os.path.join(HERE, "pullback_zt_tiny.pt"), weights_only=False)
    scfg = unet_sd.SDConfig(**tiny["cfg"])
    sp = unet_sd.init_params(scfg, seed=tiny["seed"], gain=tiny["gain"])

    class Toy:
        dtype = torch.float32

        def get_h(self, sample=None, timestep=None, encoder_hidden_states=None, op=None, block_idx=None, verbose=False):
            return unet_sd.forward(sp, scfg, sample, timestep, encoder_hidden_states, stop=(op, block_idx))

        def get_h_to_e(self, sample=None, timestep=None, encoder_hidden_states=None, input_h=None, op=None, block_idx=None, verbose=False):
            return sd_h_to_e(sp, scfg, sample, timestep, encoder_hidden_states, input_h, op, block_idx)

    toy = Toy()
    toy.local_decoder_pullback_zt = types.MethodType(ru.local_decoder_pullback_zt, toy)
    z, ctx, tt = tiny["z"], tiny["ctx"], tiny["t"]
    res = {"cfg": tiny["cfg"], "seed": tiny["seed"], "gain": tiny["gain"], "z": z, "ctx": ctx, "t": tt, "cases": []}
    for (op, idx, k, chunk, mn, mx, thr, rs) in [("mid", 0, 3, 1, 3, 30, 0.5, 41), ("down", 0, 4, 2, 1, 5, 1e-9, 42),
                                                 ("up", 0, 3, 3, 2, 30, 0.5, 43)]:
        n_h = toy.get_h(z, tt, ctx, op, idx).numel()
        (u, s, vT), it = _run(lambda: toy.local_decoder_pullback_zt(z, tt, ctx, op=op, block_idx=idx, pca_rank=k, chunk_size=chunk,
                                                                    min_iter=mn, max_iter=mx, convergence_threshold=thr), rs)
        res["cases"].append(dict(op=op, idx=idx, k=k, chunk_size=chunk, min_iter=mn, max_iter=mx, thr=thr, rng_seed=rs, V0=_v0(n_h, k, rs),
                                 iters=it, u=u.clone(), s=s.clone(), vT=vT.clone()))
        print("decoder_zt", op, idx, k, it)
    torch.save(res, os.path.join(HERE, "decoder_zt_tiny.pt"))
    for f in ("decoder_xt_ddpm.pt", "decoder_zt_tiny.pt"):
        print(f, os.path.getsize(os.path.join(HERE, f)))


if __name__ == "__main__":
    main()
