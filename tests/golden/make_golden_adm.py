"""Generate the guided-diffusion (ADM) fixtures by IMPORTING THE REFERENCE (same recipe as make_golden.py; torchvision is stubbed, einops is real):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_adm.py

Fixtures (tensors, scalars and name lists only)
  adm_toy.pt   for each toy config of tests/_adm_ref.py (T1, T2, T3): the reference's UNetModel (src/models/guided_diffusion/unet.py:398-781),
               built by its own create_model (script_util.py:379-435), with configs.adm_init_params(cfg, **init) loaded by
               load_state_dict(strict=True) -- which proves the names and shapes of configs.adm_param_shapes -- then
                 x [1, 3, S, S], xb [2, 3, S, S], t               the inputs (drawn under the recorded seed)
                 h, h_b / eps, eps_b                               UNetModel.get_h and UNetModel.forward at batch 1 and 2
                 names                                             [(name, shape)] of the reference's state_dict, in its order
               and for T1 the (u, s, vT) of the class's own local_encoder_pullback_xt (unet.py:704-781; k = 3, its default stop rule capped at
               max_iter 12) with the seed of its V0 draw; u is kept as its column norms and its first 256 rows.
               Also the parameter counts of the reference class at the two full presets (script_util.py P2_DICT / LSUN_DICT), built on the
               meta device.
Weights are regenerated from (seed, gain, spectrum) in the tests, never stored.
"""
import contextlib
import io
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from make_golden import import_reference   # noqa: E402

RNG_SEED = 1234          # torch.manual_seed before the reference draws its V0 (unet.py:735)
K, MAX_ITER = 3, 12


def reference_model(su, cfg):
    """the reference's own constructor with the arguments ADMConfig mirrors"""
    return su.create_model(image_size=cfg.image_size, num_channels=cfg.model_channels, num_res_blocks=cfg.num_res_blocks,
                           channel_mult=",".join(str(m) for m in cfg.channel_mult), learn_sigma=cfg.learn_sigma, class_cond=cfg.class_cond,
                           attention_resolutions=",".join(str(r) for r in cfg.attention_resolutions), num_heads=cfg.num_heads,
                           num_head_channels=cfg.num_head_channels, use_scale_shift_norm=cfg.use_scale_shift_norm, dropout=0.0,
                           resblock_updown=cfg.resblock_updown, use_new_attention_order=cfg.use_new_attention_order)


def main():
    import torch
    torch.set_num_threads(8)
    import_reference()
    import models.guided_diffusion.script_util as su
    import _adm_ref as R
    from diffusion_pullback_amd import configs as cf

    fix = {"toys": {}, "rng_seed": RNG_SEED, "k": K, "max_iter": MAX_ITER, "min_iter": 10, "thr": 1e-3, "chunk_size": 10}
    for name, cfg in R.TOYS.items():
        init = R.TOY_INIT[name]
        net = reference_model(su, cfg).eval()
        p = cf.adm_init_params(cfg, **R.init_kwargs(init))
        net.load_state_dict(p, strict=True)
        g = torch.Generator().manual_seed(init["input_seed"])
        s = cfg.image_size
        x, xb, t = torch.randn(1, 3, s, s, generator=g), torch.randn(2, 3, s, s, generator=g), torch.tensor(600.0)
        with torch.no_grad():
            d = dict(x=x, xb=xb, t=t, h=net.get_h(x, t).clone(), h_b=net.get_h(xb, t).clone(), eps=net(x, t).clone(), eps_b=net(xb, t).clone(),
                     names=[(k, tuple(v.shape)) for k, v in net.state_dict().items()], init=dict(init))
        print(name, "h", tuple(d["h"].shape), "eps", tuple(d["eps"].shape), "params", sum(v.numel() for v in net.state_dict().values()))
        if name == "T1":
            torch.manual_seed(RNG_SEED)
            with contextlib.redirect_stdout(io.StringIO()) as log:
                u, sv, vT = net.local_encoder_pullback_xt(x=x, t=t, op="mid", block_idx=0, pca_rank=K, chunk_size=fix["chunk_size"],
                                                          min_iter=fix["min_iter"], max_iter=MAX_ITER, convergence_threshold=fix["thr"])
            hist = [float(l.split("tensor(")[1].split(")")[0].split(",")[0]) for l in log.getvalue().splitlines() if "-th step convergence" in l]
            d.update(s=sv.clone(), vT=vT.clone(), u_norms=u.norm(dim=0).clone(), u_head=u[:256].clone(), iters=len(hist), dist_history=hist)
            print("T1 pullback:", len(hist), "iterations, s =", sv.tolist())
        fix["toys"][name] = d
    counts = {}
    for name, cfg in (("ADM_P2_256", cf.ADM_P2_256), ("ADM_LSUN_256", cf.ADM_LSUN_256)):
        with torch.device("meta"):
            net = reference_model(su, cfg)
        counts[name] = sum(v.numel() for v in net.state_dict().values())
    fix["param_counts"] = counts
    print(counts)
    out = os.path.join(HERE, "adm_toy.pt")
    torch.save(fix, out)
    print("adm_toy.pt", os.path.getsize(out))


if __name__ == "__main__":
    main()
