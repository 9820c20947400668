"""CPU-only checks of the guided-diffusion (ADM) network kind: the restatement tests/_adm_ref.py against the REFERENCE's own outputs (fixture
adm_toy.pt, tests/golden/make_golden_adm.py), the parameter tables of configs.py against the reference's state dict, the qkv repacking."""
import pytest
import torch

import _adm_ref as R
from _util import load_golden, rel
from diffusion_pullback_amd import configs as cf


@pytest.fixture(scope="module")
def fix():
    return load_golden("adm_toy.pt")


@pytest.mark.parametrize("name", ["T1", "T2", "T3"])
def test_restatement_reproduces_the_reference(fix, name):
    """fp32 relative Frobenius <= 1e-5, the bar tests/test_oracle.py holds the other restatements to"""
    f, cfg = fix["toys"][name], R.TOYS[name]
    assert f["init"] == R.TOY_INIT[name]
    p = cf.adm_init_params(cfg, **R.init_kwargs(f["init"]))
    with torch.no_grad():
        for x, h, e in ((f["x"], f["h"], f["eps"]), (f["xb"], f["h_b"], f["eps_b"])):
            eh, ee = rel(R.get_h(p, cfg, x, f["t"]), h), rel(R.forward(p, cfg, x, f["t"]), e)
            print(name, x.shape[0], "get_h", eh, "eps", ee)
            assert eh <= 1e-5 and ee <= 1e-5
        h = R.get_h(p, cfg, f["x"], f["t"])
        assert rel(R.get_h_to_e(p, cfg, f["x"], f["t"], h), f["eps"]) <= 1e-5                # continuing from the tap is the forward
        # a timestep per sample: each row is the row of the batch at that row's scalar timestep (fp32 CPU kernels depend on the batch: the 1e-5 bar)
        tt = torch.tensor([600.0, 123.0])
        hb = R.get_h(p, cfg, f["xb"], tt)
        assert rel(hb[:1], R.get_h(p, cfg, f["xb"][:1], tt[0])) <= 1e-5 and rel(hb[1:], R.get_h(p, cfg, f["xb"][1:], tt[1])) <= 1e-5


@pytest.mark.parametrize("name", ["T1", "T2", "T3"])
def test_param_shapes_equal_the_reference_state_dict(fix, name):
    shapes = cf.adm_param_shapes(R.TOYS[name])
    assert [(k, tuple(v)) for k, v in shapes.items()] == [(k, tuple(v)) for k, v in fix["toys"][name]["names"]]
    p = cf.adm_init_params(R.TOYS[name], seed=3)
    assert all(tuple(p[k].shape) == v for k, v in shapes.items())
    for k in shapes:                                   # the layers the reference zero-initialises are filled
        if k.endswith(("out_layers.3.weight", "proj_out.weight")) or k == "out.2.weight":
            assert p[k].abs().max() > 0, k


def test_param_counts_of_the_full_presets(fix):
    import math
    for name, cfg in (("ADM_P2_256", cf.ADM_P2_256), ("ADM_LSUN_256", cf.ADM_LSUN_256)):
        assert sum(math.prod(s) for s in cf.adm_param_shapes(cfg).values()) == fix["param_counts"][name]
    assert cf.ADM_P2_256.channel_mult == cf.ADM_LSUN_256.channel_mult == (1, 1, 2, 2, 4, 4)
    assert cf.ADM_P2_256.attention_ds == (16,) and cf.ADM_LSUN_256.attention_ds == (8, 16, 32)
    assert set(cf.ADM_MODEL_NAMES) == {"FFHQ_P2", "AFHQ_P2", "Flower_P2", "LSUN_bedroom", "LSUN_cat", "LSUN_horse"}


@pytest.mark.parametrize("new_order", [False, True], ids=["legacy", "new"])
def test_qkv_rows_against_the_reference_layouts(new_order):
    """The engine's fused projection is q | k | v, each [heads][d].  The reference reads head h's (q, k, v) at rows [h][3][d] of the width axis
    (QKVAttentionLegacy: reshape(bs * heads, 3 * d, L).split(d)) or at [3][heads][d] (QKVAttention: chunk(3), then the heads)."""
    c, heads = 48, 3
    d = c // heads
    rows = cf.adm_qkv_rows(c, heads, new_order)
    assert sorted(rows.tolist()) == list(range(3 * c))
    w = torch.randn(3 * c, c, generator=torch.Generator().manual_seed(0))
    x = torch.randn(c, 7, generator=torch.Generator().manual_seed(1))
    qkv = w @ x                                        # the reference's projection [3C, L]
    ours = w[rows] @ x
    for part in range(3):
        for h in range(heads):
            for j in range(d):
                src = part * c + h * d + j if new_order else h * 3 * d + part * d + j
                assert rows[part * c + h * d + j] == src
    if new_order:
        q, k, v = (a.reshape(heads, d, 7) for a in qkv.chunk(3, dim=0))
    else:
        q, k, v = qkv.reshape(heads, 3 * d, 7).split(d, dim=1)
    assert torch.equal(ours[:c].reshape(heads, d, 7), q) and torch.equal(ours[c:2 * c].reshape(heads, d, 7), k)
    assert torch.equal(ours[2 * c:].reshape(heads, d, 7), v)


def test_class_conditional_configs_are_refused():
    import dataclasses
    cfg = dataclasses.replace(R.T1, class_cond=True)
    with pytest.raises(ValueError):
        cf.adm_param_shapes(cfg)
    with pytest.raises(ValueError):
        from diffusion_pullback_amd.tape import build_adm
        build_adm(cfg, {}, torch.float32, "cpu")


def test_t1_reference_spectrum_is_separated(fix):
    """The pullback pin of tests/test_gpu_adm.py compares single vectors: at least two of the reference's three singular values must be separated
    from both neighbours by more than 5 % in the fp64 SVD of the restatement's full Jacobian -- decided by the CPU reference alone."""
    f, cfg = fix["toys"]["T1"], R.T1
    sv, _ = R.full_jacobian_svd(f, cfg)
    ok = R.separated(sv, 3)
    print("sigma", sv[:5].tolist(), "separated", ok)
    assert sum(ok) >= 2
    assert torch.allclose(f["s"].double(), sv[:3], rtol=2e-3)      # the reference's 12 capped iterations have found them
