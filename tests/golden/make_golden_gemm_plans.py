"""Records the GEMM dispatch (dpb_debug_gemm_plan: return code, kind, tile, splitk) over a fixed, seedless sweep -> tests/golden/gemm_plans.npz.

The fixture pins the dispatch across refactors of gemm.hip: generate it ONCE from a build of the commit whose dispatch is to be kept

    DPB_LIB=/path/to/that/libdpb.so python tests/golden/make_golden_gemm_plans.py <commit hash>

and tests/test_host_logic.py::test_gemm_plans_reproduce_the_recorded_dispatch replays the same sweep (sweep() / record() below are shared by the
generator and the test) against the library under test, entry for entry.  Host-only: no GPU is touched.

The sweep: the primary grid of test_gemm_dispatch_plans_... (7 tangent counts x 4 levels x 9 N x 6 K x 3 dtypes, the 3x3 convolution grid) under every
epilogue code 0..5 (3 / 4 are refused through this entry point: the refusal is the recorded return code) and three slab sizes; a ragged set; every
dpb_debug_set dispatch switch on a reduced grid; every dispatch environment switch (read once per process) in a child process each.
"""
import ctypes as C
import hashlib
import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_plans.npz")
F32, BF16, F16 = 0, 1, 2
SLABS = (64 << 20, 1 << 20, 0)
CHANS = (320, 640, 960, 1280, 1920, 2560, 3840, 5120, 10240)
RESET = {"gemm_tile": 0, "gemm_splitk": 0, "gemm_kch": 0, "p8": 1, "wres": 1, "gemm_dma_auto": 1}
FORCED = (64, 128, 129, 131, 133, 257, 65, 67, 512, 513, 514, 515, 516, 517, 518, 520, 521, 522, 523, 530, 540, 600, 519)   # 519: not a code
ENVS = ({"DPB_P8": "0"}, {"DPB_WRES": "0"}, {"DPB_WRES_MIN_M": "8192"}, {"DPB_TILE256": "0"}, {"DPB_HALF_TILE": "0"}, {"DPB_HALF_TILE": "1"},
        {"DPB_HALF_TILE": "2"}, {"DPB_HALF_KMIN": "512"}, {"DPB_CONV_HALO": "0"}, {"DPB_SPLITK_TARGET": "512"},
        {"DPB_GEMM_OVERRIDE": "320x1280x1280:0=515/4,10240x1280x5120:0=515/2,5120x640x1280:0=530/0,20480x320x320:0=540/3,1280x1280x11520:1=600/3"})
DISPATCH_ENV = ("DPB_P8", "DPB_WRES", "DPB_WRES_MIN_M", "DPB_TILE256", "DPB_HALF_TILE", "DPB_HALF_KMIN", "DPB_CONV_HALO", "DPB_SPLITK_TARGET",
                "DPB_GEMM_OVERRIDE")


def primary():
    """queries (dtype, M, N, K, conv_hw, conv_cin, epilogue, slab_bytes) of the primary grid"""
    q = []
    for slab in SLABS:
        for epi in (0, 1, 2, 5, 3, 4):
            for nt in (1, 3, 5, 10, 20, 40, 80):
                for hw in (8, 16, 32, 64):
                    M = nt * hw * hw
                    for N in CHANS:
                        for K in (320, 640, 1280, 2560, 5120, 10240):
                            for dt in (BF16, F16, F32):
                                q.append((dt, M, N, K, 0, 0, epi, slab))
                    for cin in (320, 640, 1280, 1920, 2560):
                        for cout in (320, 640, 1280):
                            q.append((BF16, M, cout, 9 * cin, hw, cin, epi, slab))
    return q


def ragged():
    return [(dt, M, N, K, 0, 0, epi, slab) for slab in SLABS for epi in (0, 1) for dt in (BF16, F32) for M in (1, 63, 64, 65, 200, 320, 321, 1000)
            for N in (8, 96, 200, 320, 328) for K in (8, 64, 200, 256, 320, 328, 512)]


def reduced():
    """the grid of the switch sweeps: every level at four tangent counts, plain and convolution, plain and GEGLU epilogue, plus the shapes the
    override string names (with ample and with scarce slab scratch) and a ragged handful"""
    q = []
    for nt in (1, 5, 20, 80):
        for hw in (8, 16, 32, 64):
            M = nt * hw * hw
            for N in (320, 640, 1280, 2560):
                for K in (320, 1280, 5120):
                    for dt in (BF16, F32):
                        for epi in (0, 1):
                            q.append((dt, M, N, K, 0, 0, epi, SLABS[0]))
            for cin in (320, 1280):
                for cout in (320, 640, 1280):
                    q.append((BF16, M, cout, 9 * cin, hw, cin, 0, SLABS[0]))
            q.append((BF16, M, 128, 9 * 64, hw, 64, 0, SLABS[0]))
    for slab in SLABS:
        q += [(BF16, 320, 1280, 1280, 0, 0, 0, slab), (BF16, 1280, 1280, 1280, 0, 0, 0, slab), (BF16, 10240, 1280, 5120, 0, 0, 0, slab),
              (BF16, 5120, 640, 1280, 0, 0, 0, slab), (F16, 20480, 320, 320, 0, 0, 0, slab), (BF16, 1280, 1280, 11520, 16, 1280, 0, slab),
              (BF16, 256, 320, 320, 0, 0, 0, slab), (F32, 256, 320, 320, 0, 0, 0, slab), (BF16, 256, 128, 576, 16, 64, 0, slab)]
    q += [(BF16, M, N, K, 0, 0, 0, SLABS[0]) for M in (65, 200, 1000) for N in (96, 200, 328) for K in (64, 200, 328, 512)]
    return q


def sweep():
    """[(env, switches, queries)]: env {} = this process, else one child process per distinct env; switches: dpb_debug_set (key, value) pairs"""
    g = [({}, (), primary() + ragged())]
    red = reduced()
    for code in FORCED:
        g.append(({}, (("gemm_tile", code),), red))
    for sk in (2, 7):
        g.append(({}, (("gemm_splitk", sk),), red))
    for code in (515, 518, 530, 540, 600, 131, 64):                       # a forced split on tiles that never split by themselves / have no slab path
        g.append(({}, (("gemm_tile", code), ("gemm_splitk", 2)), red))
    g.append(({}, (("gemm_kch", 8),), red))
    for key in ("p8", "wres", "gemm_dma_auto"):
        g.append(({}, ((key, 0),), red))
    for env in ENVS:
        g.append((env, (), red))
    return g


def sweep_hash():
    return hashlib.sha1(json.dumps(sweep(), sort_keys=True).encode()).hexdigest()


def _load_lib():
    """lib.py by path (not through the package, whose import pulls in torch: the children only need ctypes)"""
    spec = importlib.util.spec_from_file_location("_dpb_lib", os.path.join(ROOT, "diffusion_pullback_amd", "lib.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)
    return L, L.load()


def _run(L, lib, switches, queries):
    out = []
    k, t, s = C.c_int(), C.c_int(), C.c_int()
    try:
        for key, value in switches:
            L.check(lib.dpb_debug_set(key.encode(), value))
        for (dt, M, N, K, hw, cin, epi, slab) in queries:
            k.value = t.value = s.value = 0
            rc = lib.dpb_debug_gemm_plan(dt, M, N, K, hw, cin, epi, slab, C.byref(k), C.byref(t), C.byref(s))
            out.append((rc, k.value, t.value, s.value) if rc == 0 else (rc, 0, 0, 0))
    finally:
        for key, _ in switches:                                           # each switch back to its default
            L.check(lib.dpb_debug_set(key.encode(), RESET[key]))
    return out


def record():
    """the (rc, kind, tile, splitk) of every sweep entry, in sweep order, from the library lib.load() finds (DPB_LIB or the tree's)"""
    L, lib = _load_lib()
    groups, out = sweep(), []
    children = {}
    for i, (env, _, _) in enumerate(groups):                              # the environment switches are read once per process: a child each, all started at once
        if env:
            e = {k: v for k, v in os.environ.items() if k not in DISPATCH_ENV}
            e.update(env)
            children[i] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", str(i)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                           text=True, env=e, cwd=ROOT)
    for i, (env, switches, queries) in enumerate(groups):
        if env:
            so, se = children[i].communicate(timeout=300)
            assert children[i].returncode == 0, se[-2000:]
            res = [tuple(r) for r in json.loads(so.strip().splitlines()[-1])]
        else:
            res = _run(L, lib, switches, queries)
        assert len(res) == len(queries)
        out += res
    return out


def describe(index):
    """(env, switches, query) of the sweep entry at `index` -- for the message of a failing comparison"""
    for env, switches, queries in sweep():
        if index < len(queries):
            return env, switches, queries[index]
        index -= len(queries)
    raise IndexError(index)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        L, lib = _load_lib()
        _, switches, queries = sweep()[int(sys.argv[2])]
        print(json.dumps(_run(L, lib, switches, queries)))
    else:
        import numpy as np
        assert len(sys.argv) == 2, "usage: DPB_LIB=<build of the recorded commit> make_golden_gemm_plans.py <commit hash>"
        plans = np.asarray(record(), dtype=np.int16)
        assert plans.shape[1] == 4 and int(np.abs(plans).max()) < 32767
        np.savez_compressed(OUT, plans=plans, commit=np.array(sys.argv[1]), sweep=np.array(sweep_hash()))
        print(f"{OUT}: {plans.shape[0]} plans of commit {sys.argv[1]}, {os.path.getsize(OUT)} bytes")
