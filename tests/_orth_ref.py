"""Float64 reference, error measures and restatement of dpb_orth (diffusion_pullback_amd/csrc/orth.hip), and the cases its tests share.

Reference: numpy.linalg.svd of the fp32 input in float64, rows signed to overlap the previous iterate.  Every bound is a multiple of a FLOOR computed
per case: the error the float64 reference itself has once it is rounded to fp32, which is the best any fp32 output can do.  vec = 1 means "as good as
the rounded reference"; an fp32 accumulation anywhere in the method costs 65x and more (tests/test_orth_host.py keeps the two mutants failing).

The restatement follows the kernels step by step -- Gram matrix and overlaps, eigen-decomposition, descending order with ties in index order,
Cm = diag(sgn / sigma) E^T with the 1e-150 floor, V = Cm W rounded to fp32, the two convergence figures -- in numpy.  Two facts of the Jacobi solver
that LAPACK's eigh does not share are restated explicitly, because the exact cases rest on them: an index whose off-diagonal Gram entries are all
exactly zero is never rotated (its eigenvector stays the unit vector, its eigenvalue the diagonal entry, bit for bit), and equal eigenvalues keep
their index order.
"""
import functools

import numpy as np

U32 = 2.0 ** -23                 # one fp32 ulp, relative
MIN_SIGMA = 1e-150               # orth.hip: below this singular value a direction is dead (row of zeros)
MIN_OVERLAP = 1e-8               # input condition: |<V_ref[i], Vprev[i]>| of every accuracy case (below, rounding decides the sign)
MIN_GAP = 1e-3                   # input condition: relative gap of adjacent singular values
MUTANT_FACTOR = 16.0             # each fp32 mutant must miss the vec bound by at least this factor

# (k, N) of the accuracy cases at two decades, by the route they are there for (orth.hip launch_orth)
ROUTES = {
    "apply16": [(1, 64), (2, 300), (5, 1000), (6, 1000), (16, 4099)],             # cyclic k <= 5 | round-robin 256 threads; N < 256, N ragged
    "apply56": [(17, 700), (32, 520), (33, 700), (56, 2000)],                     # eig_par<32> | <64>, register-tiled apply<56>
    "tiled": [(57, 2000), (64, 520)],                                             # row-tiled apply
    "eig96": [(65, 3001), (96, 1000)],                                            # eig_par<96>
    "qglobal": [(97, 1000), (128, 200), (128, 16384)],                            # eigenvectors in global memory
    "gridstride": [(10, 65795), (24, 65795), (60, 65795), (128, 65795)],          # nbg capped at 64, nb at 256; 65795 = 65536 + 256 + 3
}
LADDER_SHAPE = (50, 16384)       # conditioning ladder: the reference's default rank
LADDER = [1, 2, 3, 4]            # decades inside the pinned domain
BEYOND = [5, 6]                  # outside it: eps64 cond^2 exceeds the fp32 floor
ACCURACY_CASES = [(k, N, 2, r) for r, shapes in ROUTES.items() for k, N in shapes] + [LADDER_SHAPE + (d, "ladder") for d in LADDER]
CONVERGED = [(5, 1000), (50, 4099), (128, 1000)]
EXACT_K = [5, 12, 40, 100]       # cyclic | round-robin 256 threads | round-robin 1024 threads | eigenvectors in global memory
DEFICIENT = [(12, 1000), (50, 1000)]
MUTANT_CASES = [(16, 4099), (56, 2000), (96, 1000)]      # one per k band of the apply kernels
# seeds: 0 unless the input conditions (MIN_OVERLAP, MIN_GAP; asserted in tests/test_orth_host.py) ask for another
SEEDS = {}


def seed_of(k, N, decades):
    return SEEDS.get((k, N, decades), 0)


def bounds(decades):
    """(vec, on) bounds in floors: 2 up to three decades, 4 at four (the float64 restatement itself measures 1.03 / 2.10 there)"""
    return (2.0, 2.0) if decades <= 3 else (4.0, 4.0)


# ----------------------------------------------------------------------------------------------------------- inputs
def _frame(rng, N, k):
    """k orthonormal rows of length N, float64"""
    return np.linalg.qr(rng.standard_normal((N, k)))[0].T


def make(k, N, decades, seed=0):
    """W = M diag(logspace(0, -decades, k)) Q^T in fp32 (Q [N][k] orthonormal, M [k][k] orthogonal) and Vprev: fp32 rows of a second random
    orthonormal basis"""
    rng = np.random.default_rng([seed, k, N, int(decades)])
    Qt = _frame(rng, N, k)
    M = np.linalg.qr(rng.standard_normal((k, k)))[0]
    W = M @ (np.logspace(0.0, -float(decades), k)[:, None] * Qt)
    Vp = _frame(rng, N, k)
    return np.ascontiguousarray(W, dtype=np.float32), np.ascontiguousarray(Vp, dtype=np.float32)


def make_converged(k, N, seed=0):
    """W = diag(sigma) Vprev in fp32, two decades: the iteration's fixed point, where the solver's stop rule fires"""
    rng = np.random.default_rng([seed, k, N, 77])
    Vp = np.ascontiguousarray(_frame(rng, N, k), dtype=np.float32)
    sig = np.logspace(0.0, -2.0, k).astype(np.float32)
    return np.ascontiguousarray(sig[:, None] * Vp), Vp


TIE_SEEDS = {5: 3}               # k = 5, sigma = (2, 1, 4, 2, 4): a shuffle on which an exchange sort that swaps rows (not stable) displaces a tie


def make_ties(k, N, seed=None):
    """W[i] = sigma_i e_{n_i}: one-hot rows at distinct columns, sigma from {4, 2, 1} in tie groups, rows shuffled.  Returns W, the expected V (the
    one-hot rows by descending sigma, ties in input order), the expected s, and Vprev = the expected V."""
    rng = np.random.default_rng([TIE_SEEDS.get(k, 0) if seed is None else seed, k, N, 78])
    sig = np.array([4.0, 2.0, 1.0])[np.arange(k) % 3][rng.permutation(k)]
    cols = rng.permutation(N)[:k]
    W = np.zeros((k, N), dtype=np.float32)
    W[np.arange(k), cols] = sig
    order = np.argsort(-sig, kind="stable")
    V = np.zeros((k, N), dtype=np.float32)
    V[np.arange(k), cols[order]] = 1.0
    return W, V, np.sqrt(sig[order]).astype(np.float32), V.copy()


def make_dead(k, N, seed=0):
    """one all-zero row (index k // 2) among k - 1 rows made as make(k - 1, N, 2): returns W, Vprev and the live rows"""
    live, _ = make(k - 1, N, 2, seed)
    _, Vp = make(k, N, 2, seed)
    W = np.insert(live, k // 2, 0.0, axis=0)
    return np.ascontiguousarray(W), Vp, live


def make_deficient(k, N, seed=0):
    """the last two rows are fp32 linear combinations of k - 2 rows made as make(k - 2, N, 2)"""
    base, _ = make(k - 2, N, 2, seed)
    _, Vp = make(k, N, 2, seed)
    rng = np.random.default_rng([seed, k, N, 79])
    c = (rng.standard_normal((2, k - 2)) / np.sqrt(k - 2)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([base, c @ base]), dtype=np.float32), Vp


# ----------------------------------------------------------------------------------------------------------- reference and floors
def svd_ref(W, Vprev):
    """numpy.linalg.svd of W in float64 -> (V_ref [k][N] rows by descending singular value, signed to a non-negative float64 overlap with the same
    row of Vprev; sqrt(S) [k])"""
    _, S, Vt = np.linalg.svd(W.astype(np.float64), full_matrices=False)
    ov = np.einsum("ij,ij->i", Vt, Vprev.astype(np.float64))
    Vt[ov < 0] *= -1.0
    return Vt, np.sqrt(S)


def floors(V_ref):
    """(floor_vec [k], floor_on): what rounding the float64 reference to fp32 costs, per row and in orthonormality"""
    Vi = V_ref.astype(np.float32).astype(np.float64)
    return np.linalg.norm(Vi - V_ref, axis=1), np.abs(Vi @ Vi.T - np.eye(len(Vi))).max()


def input_conditions(W, Vprev, V_ref, sqrtS):
    """(smallest |<V_ref[i], Vprev[i]>|, smallest relative gap of adjacent singular values)"""
    ov = np.abs(np.einsum("ij,ij->i", V_ref, Vprev[:len(V_ref)].astype(np.float64))).min()
    S = sqrtS ** 2
    gap = ((S[:-1] - S[1:]) / S[:-1]).min() if len(S) > 1 else np.inf
    return float(ov), float(gap)


class Case:
    """an input with its float64 reference and floors, computed once"""

    def __init__(self, W, Vprev, rows=None):
        self.W, self.Vprev = W, Vprev
        self.V_ref, self.sqrtS = svd_ref(W, Vprev)
        if rows is not None:                      # only the leading rows are pinned
            self.V_ref, self.sqrtS = self.V_ref[:rows], self.sqrtS[:rows]
        self.floor_vec, self.floor_on = floors(self.V_ref)
        for a in (self.W, self.Vprev, self.V_ref, self.sqrtS, self.floor_vec):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def inputs(k, N, decades):
    W, Vp = make(k, N, decades, seed_of(k, N, decades))
    W.setflags(write=False); Vp.setflags(write=False)
    return W, Vp


@functools.lru_cache(maxsize=None)
def case(k, N, decades):
    return Case(*inputs(k, N, decades))


@functools.lru_cache(maxsize=None)
def converged_case(k, N):
    return Case(*make_converged(k, N))


@functools.lru_cache(maxsize=None)
def dead_case(k, N):
    W, Vp, live = make_dead(k, N)
    c = Case(live, Vp[:k - 1])
    c.W_full, c.Vprev_full = W, Vp
    return c


@functools.lru_cache(maxsize=None)
def deficient_case(k, N):
    W, Vp = make_deficient(k, N)
    return Case(W, Vp, rows=k - 2)


# ----------------------------------------------------------------------------------------------------------- measures
def conv_recomputed(V, Vprev):
    """(conv0, conv1, max|d|) in float64 from the RETURNED V: d = float32(Vprev - V), one fp32 subtraction as in the kernel; conv0 = sqrt(sum d^2),
    conv1 = max(0, max(|d| - float32(1e-5) |V|)).  (Not an fp32 restatement of conv1: the compiler may contract the kernel's expression to an fma.)"""
    d = (Vprev.astype(np.float32) - V.astype(np.float32)).astype(np.float64)
    viol = np.abs(d) - float(np.float32(1e-5)) * np.abs(V.astype(np.float64))
    return float(np.sqrt((d * d).sum())), float(max(0.0, viol.max())), float(np.abs(d).max())


def measure(V, s, conv, c, Vprev=None):
    """errors of a result (V [r][N], s [r], conv [2]) against Case c, r = its pinned rows; Vprev: the previous iterate conv was computed from (all
    rows), default c.Vprev.  Returns a dict: vec (worst row, in floors), on (in floors), s_ulps (worst), conv0_ulps, conv1_err, dmax, overlap (smallest
    float64 overlap of a row with Vprev)."""
    r = len(c.V_ref)
    V64 = np.asarray(V, dtype=np.float64)
    Vp = c.Vprev if Vprev is None else Vprev
    vec = np.linalg.norm(V64[:r] - c.V_ref, axis=1) / c.floor_vec
    on = np.abs(V64[:r] @ V64[:r].T - np.eye(r)).max() / c.floor_on
    s64 = np.asarray(s, dtype=np.float64)[:r]
    s_ulps = np.abs(s64 - c.sqrtS) / (U32 * c.sqrtS)
    c0, c1, dmax = conv_recomputed(np.asarray(V), Vp)
    conv = np.asarray(conv, dtype=np.float64)
    conv0_ulps = abs(conv[0] - c0) / (U32 * c0) if c0 > 0 else (0.0 if conv[0] == 0 else np.inf)
    return dict(vec=float(vec.max()), on=float(on), s_ulps=float(s_ulps.max()), s_ulps_rows=s_ulps, conv0_ulps=float(conv0_ulps),
                conv1_err=float(abs(conv[1] - c1)), dmax=dmax,
                overlap=float(np.einsum("ij,ij->i", V64[:r], Vp[:r].astype(np.float64)).min()))


def line(k, N, decades, route, m):
    return (f"ORTH-ERR {k} {N} {decades} {route} {m['vec']:.3f} {m['on']:.3f} {m['s_ulps']:.3f} {m['conv0_ulps']:.3f} "
            f"{m['conv1_err']:.2e}")


def check(V, s, conv, c, k, N, decades, route, Vprev=None):
    """prints the ORTH-ERR line of a result, then asserts every bound of the pinned domain; returns the measures"""
    m = measure(V, s, conv, c, Vprev)
    print(line(k, N, decades, route, m))
    what = f"k={k} N={N} decades={decades} {route}"
    bv, bo = bounds(decades)
    assert np.isfinite(np.asarray(V)).all() and np.isfinite(np.asarray(s)).all() and np.isfinite(np.asarray(conv)).all(), what
    assert m["vec"] <= bv, (what, "vec", m["vec"])
    assert m["on"] <= bo, (what, "on", m["on"])
    assert m["s_ulps"] <= 1.0, (what, "s_ulps", m["s_ulps"])
    assert m["overlap"] >= -1e-9, (what, "overlap", m["overlap"])
    assert m["conv0_ulps"] <= 1.0, (what, "conv0_ulps", m["conv0_ulps"])
    assert m["conv1_err"] <= U32 * m["dmax"], (what, "conv1_err", m["conv1_err"], m["dmax"])
    return m


# ----------------------------------------------------------------------------------------------------------- the method, restated
def _eig_jacobi_like(G):
    """eigen-decomposition of the symmetric G as the Jacobi kernels leave it: indices with an exactly zero off-diagonal row are their own eigenpairs,
    untouched; the coupled block goes through eigh.  Returns (lam [k], E [k][k] columns) in index order of the diagonal they end on -- for the
    coupled block, eigh's ascending order reversed."""
    k = len(G)
    off = G - np.diag(np.diag(G))
    coupled = np.flatnonzero(np.abs(off).sum(axis=1) > 0)
    lam, E = np.diag(G).copy(), np.eye(k)
    if len(coupled):
        l, e = np.linalg.eigh(G[np.ix_(coupled, coupled)])
        lam[coupled] = l[::-1]
        E[np.ix_(coupled, coupled)] = e[:, ::-1]
    return lam, E


def restate(W, Vprev, gram_dtype=np.float64, apply_dtype=np.float64):
    """dpb_orth in numpy -> (V fp32 [k][N], s fp32 [k], conv fp32 [2]).  gram_dtype: the type W is multiplied and accumulated in for the Gram matrix
    and the overlaps; apply_dtype: the same for V = Cm W.  float64 for both is the method; float32 for either is a mutant."""
    Wg, Vg = W.astype(gram_dtype), Vprev.astype(gram_dtype)
    G = (Wg @ Wg.T).astype(np.float64)
    X = (Wg @ Vg.T).astype(np.float64)            # X[j][i] = W_j . Vprev_i
    lam, E = _eig_jacobi_like(0.5 * (G + G.T))
    order = np.argsort(-lam, kind="stable")       # descending, ties by index
    lam, E = lam[order], E[:, order]
    sig = np.sqrt(np.maximum(lam, 0.0))
    inv = np.where(sig > MIN_SIGMA, 1.0 / np.where(sig > MIN_SIGMA, sig, 1.0), 0.0)
    dot = np.einsum("ji,ji->i", E * inv[None, :], X)
    Cm = (np.where(dot < 0, -1.0, 1.0) * inv)[:, None] * E.T
    V = (Cm.astype(apply_dtype) @ W.astype(apply_dtype)).astype(np.float32)
    d = Vprev.astype(np.float32) - V
    conv0 = np.float32(np.sqrt((d.astype(np.float64) ** 2).sum()))
    conv1 = np.float32(max(np.float32(0), (np.abs(d) - np.float32(1e-5) * np.abs(V)).max()))      # fp32, as the kernel is written
    return V, np.sqrt(sig).astype(np.float32), np.array([conv0, conv1], dtype=np.float32)


# ----------------------------------------------------------------------------------------------------------- the kernel, called
def gpu_orth(W, Vprev, inplace=False, device="cuda:0"):
    """dpb_orth_checked on fp32 numpy (or device torch) inputs -> numpy (V, s, conv); inplace: V aliases Vprev"""
    import ctypes as C

    import torch

    from diffusion_pullback_amd import lib as L
    lib = L.load()
    dev = lambda a: a.to(device) if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).to(device)
    Wd, Vpd = dev(W), dev(Vprev)
    k, n = Wd.shape
    Vpd = Vpd.clone() if inplace else Vpd
    V = Vpd if inplace else torch.empty_like(Wd)
    s = torch.empty(k, dtype=torch.float32, device=device)
    conv = torch.empty(2, dtype=torch.float32, device=device)
    scratch = torch.empty(int(lib.dpb_orth_scratch_bytes(k, n)) // 8, dtype=torch.float64, device=device)
    L.check(lib.dpb_orth_checked(Wd.data_ptr(), Vpd.data_ptr(), V.data_ptr(), s.data_ptr(), conv.data_ptr(), scratch.data_ptr(), scratch.numel() * 8,
                                 k, n, C.c_void_p(torch.cuda.current_stream(device).cuda_stream)))
    torch.cuda.synchronize(device)
    return V.cpu().numpy(), s.cpu().numpy(), conv.cpu().numpy()
