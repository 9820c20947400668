"""Generate the global-PCA / inverse-Jacobian golden fixture by IMPORTING THE REFERENCE (same recipe as make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pca.py

Fixture (tensors only)
  pca_zt_tiny.pt   utils.global_pca_zt (utils.py:978-1027) and utils.inv_jac_zt (utils.py:1117-1160) bound onto the toy SD net of
                   pullback_zt_tiny.pt (get_h = oracle.unet_sd's forward).  Every PCA case records the seed of the samples zt (redrawn by
                   tests/_pca_ref.golden_zt, checked by their sums), the RNG seed set before the call, the Gaussian matrix R that torch.pca_lowrank draws under that seed (stored when
                   N < D; redrawn by tests/_pca_ref.golden_R and checked by its sums when N >= D) (torch.randn(A.shape[-1], q) of _svd_lowrank's A:
                   [N, q] if N < D, else [D, q]) and the returned (u [D, q], s [q]).  The inv_jac_zt cases record u and the returned vT.
Regenerating reproduces the file bit for bit (CPU, fixed seeds, 8 threads).
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from make_golden import import_reference   # noqa: E402
from _pca_ref import golden_zt   # noqa: E402


def main():
    import contextlib
    import io
    import torch
    torch.set_num_threads(8)
    ru, _ = import_reference()
    from oracle import unet_sd

    tiny = torch.load(os.path.join(HERE, "pullback_zt_tiny.pt"), weights_only=False)
    scfg = unet_sd.SDConfig(**tiny["cfg"])
    sp = unet_sd.init_params(scfg, seed=tiny["seed"], gain=tiny["gain"])

    class Toy:
        dtype = torch.float32
        device = torch.device("cpu")

        def get_h(self, sample=None, timestep=None, encoder_hidden_states=None, op=None, block_idx=None, verbose=False):
            return unet_sd.forward(sp, scfg, sample, timestep, encoder_hidden_states, stop=(op, block_idx))

    toy = Toy()
    toy.global_pca_zt = types.MethodType(ru.global_pca_zt, toy)
    toy.inv_jac_zt = types.MethodType(ru.inv_jac_zt, toy)
    z, ctx, tt = tiny["z"], tiny["ctx"], tiny["t"]
    res = {"cfg": tiny["cfg"], "seed": tiny["seed"], "gain": tiny["gain"], "z": z, "ctx": ctx, "t": tt, "pca": [], "inv": []}
    # (op, idx, N, memory_bound, q, zt seed, rng seed): mid has D = 1024.  N < D at q = 1, 8, 32 (memory_bound 7 does not divide N = 40);
    # N = 1040 >= D takes the other orientation of _svd_lowrank.
    for (op, idx, n, mb, q, zs, rs) in [("mid", 0, 40, 5, 1, 51, 61), ("mid", 0, 40, 7, 8, 51, 62), ("mid", 0, 40, 5, 32, 51, 63),
                                        ("mid", 0, 1040, 100, 8, 52, 64)]:
        zt = golden_zt(dict(n=n, zt_seed=zs))
        d = toy.get_h(zt[:1], tt, ctx, op, idx).numel()
        torch.manual_seed(rs)
        with contextlib.redirect_stdout(io.StringIO()):
            u, s = toy.global_pca_zt(zt, tt, ctx, op=op, block_idx=idx, memory_bound=mb, pca_rank=q)
        torch.manual_seed(rs)
        R = torch.randn(min(n, d), q)                       # what get_approximate_basis drew inside the call
        # zt is not stored (its size): tests/_pca_ref.golden_zt redraws it from zt_seed and checks it against zt_sum
        # (nor the [D, q] R of the N >= D case: tests/_pca_ref.golden_R redraws it from rng_seed and checks it against R_sum)
        case = dict(op=op, idx=idx, n=n, d=d, memory_bound=mb, q=q, niter=5, zt_seed=zs, zt_sum=zt.double().sum().item(),
                    zt_abs_sum=zt.double().abs().sum().item(), rng_seed=rs, u=u.clone(), s=s.clone())
        if n < d:
            case["R"] = R
        else:
            case.update(R_sum=R.double().sum().item(), R_abs_sum=R.double().abs().sum().item())
        res["pca"].append(case)
        print("global_pca_zt", op, idx, n, q, s[:4].tolist())
    # inv_jac_zt at the tiny net's single sample: the top direction of the q = 8 case and a random unit direction
    u0 = res["pca"][1]["u"][:, 0].clone()
    ur = torch.randn(1024, generator=torch.Generator().manual_seed(71))
    ur = ur / ur.norm()
    for name, u in (("pc0", u0), ("random", ur)):
        vT = toy.inv_jac_zt(z, tt, ctx, op="mid", block_idx=0, u=u, perturb_h=1e-1)
        res["inv"].append(dict(name=name, op="mid", idx=0, u=u, perturb_h=1e-1, vT=vT.clone()))
        print("inv_jac_zt", name, vT.shape)
    torch.save(res, os.path.join(HERE, "pca_zt_tiny.pt"))
    print("pca_zt_tiny.pt", os.path.getsize(os.path.join(HERE, "pca_zt_tiny.pt")))


if __name__ == "__main__":
    main()
