"""Generate the h-space-shift golden fixture by IMPORTING THE REFERENCE (same recipe as make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_hshift.py

Fixture (tensors only)
  hshift_ddpm.pt   PullBackDDPM.forward(x, t, u, op, block_idx) (diffusion.py:145-200) of the reduced-width vendored DDPM of ddpm_small.pt
                   (weights = oracle.unet_ddpm.init_params(cfg, seed)) at ('mid', 0) and every ('up', i): eps of the net with u added to the
                   activation at the tap, for B = 1 (x) and B = 2 (xb), ONE u [1, C, H, W] broadcast over the batch.
The reference's 'down' branch builds a 5-D tensor (u.view(-1, *hs[-1].shape), diffusion.py:171) and cannot run: down taps are covered by the
CPU restatement (tests/_decoder_ref.py) alone.  Every case records the seed u was drawn from, u itself and the two results.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from make_golden import import_reference   # noqa: E402


def main():
    import torch
    torch.set_num_threads(8)
    ru, rd = import_reference()
    from oracle import unet_ddpm

    small = torch.load(os.path.join(HERE, "ddpm_small.pt"), weights_only=False)
    cfgd = small["cfg"]
    cfg = unet_ddpm.DDPMConfig(**cfgd)
    ns = ru.dict2namespace({"config": {"model": dict(ch=cfgd["ch"], out_ch=cfgd["out_ch"], ch_mult=list(cfgd["ch_mult"]),
                                                   num_res_blocks=cfgd["num_res_blocks"], attn_resolutions=list(cfgd["attn_resolutions"]),
                                                   dropout=0.0, in_channels=cfgd["in_channels"], resamp_with_conv=True),
                                      "data": dict(image_size=cfgd["resolution"])}})
    ns.device = "cpu"; ns.dtype = torch.float32
    net = rd.PullBackDDPM(ns).eval()
    net.load_state_dict(unet_ddpm.init_params(cfg, seed=small["seed"]), strict=True)
    x, xb, t = small["x"], small["xb"], small["t"]
    fix = {"cfg": cfgd, "seed": small["seed"], "x": x, "xb": xb, "t": t, "cases": []}
    taps = [("mid", 0)] + [("up", i) for i in reversed(range(len(cfgd["ch_mult"])))]
    with torch.no_grad():
        assert (net(x, t) - small["eps"]).abs().max() < 1e-5              # the unshifted forward is ddpm_small.pt's
        for n, (op, idx) in enumerate(taps):
            h = net.get_h(x, t, op=op, block_idx=idx)
            rs = 51 + n
            u = 0.5 * h.std() * torch.randn(1, *h.shape[1:], generator=torch.Generator().manual_seed(rs))   # a shift of half the tap's spread
            e1 = net(x, t, u=u, op=op, block_idx=idx)
            e2 = net(xb, t, u=u, op=op, block_idx=idx)
            assert (e1 - small["eps"]).norm() / small["eps"].norm() > 1e-2, "the shift does not reach eps"
            fix["cases"].append(dict(op=op, idx=idx, rng_seed=rs, u=u.clone(), eps=e1.clone(), eps_b=e2.clone()))
            print("hshift", op, idx, tuple(u.shape), float((e1 - small["eps"]).norm() / small["eps"].norm()))
        try:                                                               # the 'down' branch of the reference: recorded as not runnable
            net(x, t, u=torch.zeros(1, *small["h_down_0"].shape[1:]), op="down", block_idx=0)
            fix["down_runs"] = True
        except RuntimeError:
            fix["down_runs"] = False
    print("reference 'down' branch runs:", fix["down_runs"])
    torch.save(fix, os.path.join(HERE, "hshift_ddpm.pt"))
    print("hshift_ddpm.pt", os.path.getsize(os.path.join(HERE, "hshift_ddpm.pt")))


if __name__ == "__main__":
    main()
