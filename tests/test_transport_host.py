"""CPU checks of the parallel-transport job (dpb_transport_directions, geometry.transport_directions, run_edit_parallel_transport): the float64
restatement of the direction arithmetic against the tensors the reference's own run handed to save_image (tests/golden/make_golden_transport.py), the
names and skip rules of the job, the CLI flags, and the argument checks of the new entry points, which run before any GPU call."""
import ctypes
import os

import pytest
import torch

from _transport_ref import ref_transport
from _util import load_golden, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fixture():
    return load_golden("transport_uncond_small.pt")


def test_restatement_reproduces_the_reference_directions():
    """the vk- tensors of the reference's run, [+transported, -transported, +original, -original] per pc, computed there in fp32 from the normalised
    bases: the fp64 restatement on the same bases agrees to 1e-5 relative, and the share of each source direction the target holds is <= 1"""
    f = _fixture()
    saved = dict(f["saved"])
    u0, u1 = (u.t() for u in f["u"])
    vT0, vT1 = f["vT"]
    vk, coef, coef_norm, _ = ref_transport(u0, u1, vT1)
    assert tuple(vk.shape) == (1, 4, 3 * 32 * 32) and tuple(coef.shape) == (1, 4, 4)
    v0 = vT0.double() / vT0.double().norm(dim=1, keepdim=True)
    for pc in range(f["args"]["vis_num_pc"]):
        ref = saved[f"vk-sample_idx_0_0-sample_idx_1_1-pc_{pc:03d}.png"].reshape(4, -1)
        want = torch.stack([vk[0, pc], -vk[0, pc], v0[pc], -v0[pc]])
        errs = [rel(want[i], ref[i]) for i in range(4)]
        print(f"pc {pc}: relative error of the restatement against the reference's fp32 directions {errs}")
        assert max(errs) <= 1e-5
    print("coef_norm", coef_norm.tolist())
    assert float(coef_norm.max()) <= 1 + 1e-6 and float(coef_norm.min()) > 0
    assert torch.allclose(vk.norm(dim=2), torch.ones(1, 4, dtype=torch.float64), atol=1e-12)


def _driver(tmp, f, **kw):
    from diffusion_pullback_amd import main as m
    from diffusion_pullback_amd.edit import EditUncondDiffusion
    a = f["args"]
    argv = ["--note", "t", "--model_name", a["model_name"], "--dataset_name", a["dataset_name"], "--result_folder", str(tmp), "--device", "cpu",
            "--performance_boosting_t", "0.2", "--h_t", str(a["h_t"]), "--edit_t", str(a["edit_t"]), "--seed", str(a["seed"])]
    args = m.preset(m.parse_args(argv))
    args.for_steps = args.inv_steps = a["for_steps"]
    args.input_root = os.path.join(str(tmp), "inputs")
    for k, v in kw.items():
        setattr(args, k, v)
    return args, EditUncondDiffusion(args, unet=None)


def test_names_are_the_references_and_a_finished_job_is_skipped(tmp_path):
    f = _fixture()
    args, ed = _driver(tmp_path, f)
    i0, targets, pcs, h_t, plan = ed.parallel_transport_plan(0, 1, op="mid", block_idx=0, vis_num_pc=f["args"]["vis_num_pc"])
    assert (i0, targets, pcs, h_t) == (0, [1], [0, 1], 0.8)
    names = []
    for runs, vk_files in plan:                               # the order the sequential path writes in
        names += [f"x0_gen-{name}.png" for name, _, _ in runs] + vk_files
    assert names == [n for n, _ in f["saved"] if n.startswith(("x0_gen-", "vk-"))]
    assert [(d, s) for _, d, s in plan[0][0]] == [(0, 1), (0, -1), (None, 1), (None, -1)]
    # several targets: every target's names, the source's once
    _, targets, _, _, plan3 = ed.parallel_transport_plan(0, [1, 5], vis_num_pc=1, vis_pc_list=[3], h_t=0.5)
    runs, vk_files = plan3[0]
    assert targets == [1, 5] and len(plan3) == 1 and len(runs) == 6
    assert [n.split("-h_")[0] for n, _, _ in runs] == ["xt-CelebA_HQ-sample_idx_0_0-sample_idx_1_1"] * 2 + ["xt-CelebA_HQ-sample_idx_0_0-sample_idx_1_5"] * 2 \
        + ["xt-CelebA_HQ-sample_idx_0_0-sample_idx_1_0"] * 2
    assert all(n.endswith(("-h_0.5T-edit_0.6T-mid-block_0-seed_0-pc_003_pos", "-h_0.5T-edit_0.6T-mid-block_0-seed_0-pc_003_neg")) for n, _, _ in runs)
    assert vk_files == ["vk-sample_idx_0_0-sample_idx_1_1-pc_003.png", "vk-sample_idx_0_0-sample_idx_1_5-pc_003.png"]
    # the job's skip rule: once the last pc's _neg picture exists nothing runs -- this driver has no U-Net, dataset or GPU to run anything with
    last_neg = [n for n, _ in f["saved"] if n.startswith("x0_gen-") and "sample_idx_1_1-" in n][-1]
    assert last_neg.endswith("pc_001_neg.png")
    open(os.path.join(args.result_folder, last_neg), "w").close()
    assert ed.run_edit_parallel_transport(0, 1, vis_num=4, vis_num_pc=2, pca_rank=4) is None
    assert os.listdir(args.obs_folder) == [] and os.listdir(args.result_folder) == [last_neg] and not os.path.exists(args.input_root)
    with pytest.raises(Exception):                            # a list with an unfinished target is not skipped (and cannot run here)
        ed.run_edit_parallel_transport(0, [1, 2], vis_num=4, vis_num_pc=2, pca_rank=4)


def test_basis_files_are_the_sampling_jobs(tmp_path):
    """with --dataset_name Random the job consumes what run_sample_encoder_local_tangent_space_zt wrote, and the reverse"""
    f = _fixture()
    args, ed = _driver(tmp_path, f, dataset_name="Random")
    save_dir, exp_name = ed._tangent_space_naming("mid", 0, 50)
    assert os.path.basename(save_dir) == "local_encoder_pullback_uncond-model_CelebA_HQ_HF-dataset_Random-num_steps_20-pca_rank_50"
    assert exp_name(3, 0.8) == "xt-Random_3-0.8T-mid-block_0-seed_0"
    ref = [n.replace("CelebA_HQ", "Random") for n in f["basis_files"]]      # the names the reference's job loaded (its directory differs: scheduler_name)
    assert sorted(os.path.basename(p) for i in (0, 1) for p in ed._basis_paths(save_dir, exp_name(i, 0.8)) if "s-" not in os.path.basename(p)[:2]) == ref


def test_cli_flags_parse(capsys):
    from diffusion_pullback_amd import main as m
    a = m.parse_args(["--note", "t"])
    assert a.run_edit_parallel_transport is False and a.sample_idx_0 == 0 and a.sample_idx_1 == 0 and a.sample_idx_1_values == [0]
    a = m.parse_args(["--note", "t", "--run_edit_parallel_transport", "True", "--sample_idx_0", "3", "--sample_idx_1", "7", "--model_name", "CelebA_HQ_HF",
                      "--h_t", "0.6", "--edit_t", "0.4", "--op", "mid", "--block_idx", "0", "--pca_rank", "50", "--vis_num", "5", "--vis_num_pc", "3"])
    assert a.run_edit_parallel_transport is True and (a.sample_idx_0, a.sample_idx_1, a.sample_idx_1_values) == (3, 7, [7])
    assert (a.h_t, a.edit_t, a.pca_rank, a.vis_num, a.vis_num_pc) == (0.6, 0.4, 50, 5, 3)
    a = m.parse_args(["--note", "t", "--run_edit_parallel_transport", "True", "--sample_idx_1_list", "4, 2,9"])
    assert a.sample_idx_1_values == [4, 2, 9]
    with pytest.raises(SystemExit):
        m.parse_args(["--note", "t", "--sample_idx_1_list", "1,x"])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        m.parse_args(["--note", "t", "--run_edit_parallel_transport", "True", "--model_name", "runwayml/stable-diffusion-v1-5"])
    err = capsys.readouterr().err
    assert "Stable Diffusion" in err and "unconditional" in err
    for flag in ("--run_edit_parallel_transport", "--sample_idx_0", "--sample_idx_1", "--sample_idx_1_list"):
        assert flag in m.__doc__


def test_engine_sizing_covers_the_basis_group_and_the_chain_call(tmp_path):
    from diffusion_pullback_amd import main as m
    argv = ["--note", "t", "--model_name", "CelebA_HQ_HF", "--dataset_name", "Random", "--result_folder", str(tmp_path), "--device", "cpu",
            "--performance_boosting_t", "0.2", "--run_edit_parallel_transport", "True", "--sample_idx_1_list", "1,2,3", "--pca_rank", "50"]
    a = m.preset(m.parse_args(argv))
    assert m.transport_group(a) == 2                          # four samples at pca_rank 50: the tangent budget takes two at a time
    a.pca_rank = 10
    assert m.transport_group(a) == 4
    a.memory_bound = 3
    assert m.transport_group(a) == 3


def _lib():
    from diffusion_pullback_amd import lib
    return lib, lib.load()


def test_symbols_are_exported_and_declared():
    lib, so = _lib()
    header = open(os.path.join(ROOT, "include", "dpb.h")).read()
    for name in ("dpb_transport_directions", "dpb_transport_scratch_bytes"):
        assert name in lib.SYMBOLS and getattr(so, name) is not None and name in header, name
    assert so.dpb_abi_version() == 1


def test_scratch_bytes_is_zero_for_invalid_arguments():
    _, so = _lib()
    f = so.dpb_transport_scratch_bytes
    r = lambda b: (b + 255) // 256 * 256
    # the overlaps, three sets of row sums, the streaming coefficients, the per-chunk partial norms (1024 columns per chunk) and the scales
    assert f(3, 2, 5, 4096, 3000) == r(3 * 25 * 8) + r(5 * 8) + 2 * r(15 * 8) + r(3 * 2 * 5 * 4) + r(3 * 2 * 3 * 8) + r(3 * 2 * 4)
    assert f(1, 1, 1, 1, 1) > 0 and f(65535, 128, 128, 5, 7) > 0
    for d, p, k, nh, nx in [(1, 1, 0, 16, 16), (1, 1, 129, 4096, 4096), (1, 5, 4, 16, 16), (1, 0, 4, 16, 16), (0, 1, 4, 16, 16), (65536, 1, 4, 16, 16),
                            (1, 1, 4, 0, 16), (1, 1, 4, 16, 0), (-1, 1, 4, 16, 16)]:
        assert f(d, p, k, nh, nx) == 0, (d, p, k, nh, nx)


def test_entry_point_refuses_bad_arguments_with_a_message():
    """every check below happens on the host, before the first launch: no GPU is needed (the pointers are never dereferenced)"""
    _, so = _lib()
    fake = ctypes.c_void_p(1 << 20)               # non-null, 256-byte aligned, never touched
    err = lambda: so.dpb_last_error().decode()
    pcs = lambda *v: (ctypes.c_int32 * len(v))(*v)
    call = lambda p, P, D, k, scratch=fake, nbytes=1 << 30, **kw: so.dpb_transport_directions(
        kw.get("u_src", fake), fake, fake, p, P, D, k, 64, 96, kw.get("vk", fake), fake, fake, scratch, nbytes, None)
    need = so.dpb_transport_scratch_bytes(2, 2, 4, 64, 96)
    assert call(pcs(0), 1, 2, 0) != 0 and "k=0" in err()
    assert call(pcs(0), 1, 2, 129) != 0 and "k=129" in err()
    assert call(pcs(0, 1, 2, 3, 0), 5, 2, 4) != 0 and "P=5" in err()
    assert call(pcs(0), 0, 2, 4) != 0 and "P=0" in err()
    assert call(pcs(0, 4), 2, 2, 4) != 0 and "pcs[1]=4" in err()
    assert call(pcs(-1, 1), 2, 2, 4) != 0 and "pcs[0]=-1" in err()
    assert call(pcs(0, 1), 2, 0, 4) != 0 and "D=0" in err()
    assert call(pcs(0, 1), 2, 65536, 4) != 0 and "D=65536" in err()
    assert call(pcs(0, 1), 2, 2, 4, nbytes=need - 1) != 0 and "scratch" in err() and str(need) in err()
    assert call(pcs(0, 1), 2, 2, 4, scratch=ctypes.c_void_p((1 << 20) + 8), nbytes=need) != 0 and "aligned" in err()
    assert call(None, 2, 2, 4) != 0 and "null" in err()
    assert call(pcs(0, 1), 2, 2, 4, u_src=None) != 0 and "null" in err()
    assert call(pcs(0, 1), 2, 2, 4, vk=None) != 0 and "null" in err()
    assert call(pcs(0, 1), 2, 2, 4, scratch=None) != 0 and "null" in err()


def test_geometry_refuses_cpu_tensors_and_bad_shapes():
    from diffusion_pullback_amd import geometry
    from diffusion_pullback_amd.lib import DpbError
    with pytest.raises(DpbError, match="no CPU fallback"):
        geometry.transport_directions(torch.zeros(3, 8), torch.zeros(3, 8), torch.zeros(3, 16))
