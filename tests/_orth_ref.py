"""Float64 reference, error measures and restatement of dpb_orth (diffusion_pullback_amd/csrc/orth.hip), and the cases its tests share.

Reference: numpy.linalg.svd of the fp32 input in float64, rows signed to overlap the previous iterate.  Every bound is a multiple of a FLOOR computed
per case: the error the float64 reference itself has once it is rounded to fp32, which is the best any fp32 output can do.  vec = 1 means "as good as
the rounded reference"; an fp32 accumulation anywhere in the method costs 65x and more (tests/test_orth_host.py keeps the two mutants failing).

The restatement follows the kernels step by step -- Gram matrix and overlaps, eigen-decomposition, descending order with ties in index order,
Cm = diag(sgn / sigma) E^T with the 1e-150 floor, V = Cm W rounded to fp32, the two convergence figures -- in numpy.  Two facts of the Jacobi solver
that LAPACK's eigh does not share are restated explicitly, because the exact cases rest on them: an index whose off-diagonal Gram entries are all
exactly zero is never rotated (its eigenvector stays the unit vector, its eigenvalue the diagonal entry, bit for bit), and equal eigenvalues keep
their index order.

Non-finite input has a rule of its own (include/dpb.h at dpb_orth), restated here too: a NaN or an inf in W gives V, s and conv all NaN; a non-finite
Vprev leaves s and |V| alone and gives conv = (NaN, NaN); the eigenvalue ranking is a total order (rank_scatter) and conv[1] keeps a NaN (max_nan).
The cases (NF_*), the poisons and the two assertions are shared by tests/test_gpu_orth.py and tests/test_orth_host.py, which also keeps the three
traits the kernels had before the rule (MUTANTS) failing those assertions.
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


POISON = -1                      # what a slot of `order` holds before the rank scatter
STALE = 1.0                      # what the restatement reads through a slot the scatter never wrote: a finite number, "whatever the memory held"
MUTANTS = ("rank_plain", "clamp", "fmax")


def rank_scatter(lam, total=True):
    """order[rank(lam, t)] = t for every t into an array of POISON, as eig_par_kernel does it.  total: the order of sorts_before (csrc/rank.h) --
    descending, NaN first, ties by index; otherwise the plain comparison lam[e] > lam[t] or (== and e < t), under which a NaN counts nothing and is
    counted by nothing."""
    k = len(lam)
    order = np.full(k, POISON, dtype=np.int64)
    for t in range(k):
        mine, rank = lam[t], 0
        for e in range(k):
            if total and (np.isnan(lam[e]) or np.isnan(mine)):
                rank += bool(np.isnan(lam[e]) and (not np.isnan(mine) or e < t))
            else:
                rank += bool(lam[e] > mine or (lam[e] == mine and e < t))
        order[rank] = t
    return order


def max_nan(a, b):
    """the kernels' maximum of the convergence figure: keeps a NaN operand (Python's max(0, nan) is 0, as fmaxf's)"""
    return np.maximum(a, b)


def restate(W, Vprev, gram_dtype=np.float64, apply_dtype=np.float64, mutant=None):
    """dpb_orth in numpy -> (V fp32 [k][N], s fp32 [k], conv fp32 [2]).  gram_dtype: the type W is multiplied and accumulated in for the Gram matrix
    and the overlaps; apply_dtype: the same for V = Cm W.  float64 for both is the method; float32 for either is a mutant.

    Non-finite input, the rule of include/dpb.h: a NaN or an inf in W (read off the Gram diagonal) gives V, s and conv all NaN without an eigen-solve;
    a non-finite Vprev only reaches the sign alignment and conv, where an inf difference counts as NaN and both figures propagate it.
    mutant (one of MUTANTS) restates the method WITHOUT that detection and with one of the three traits it had before the rule: "rank_plain" ranks
    the eigenvalues by the plain comparison into a poisoned `order` and reads STALE through the unwritten slots, "clamp" takes lam > 0 ? lam : 0,
    "fmax" takes the maximum of conv[1] with a NaN-dropping max."""
    assert mutant is None or mutant in MUTANTS
    k = len(W)
    with np.errstate(all="ignore"):
        Wg, Vg = W.astype(gram_dtype), Vprev.astype(gram_dtype)
        G = (Wg @ Wg.T).astype(np.float64)
        X = (Wg @ Vg.T).astype(np.float64)            # X[j][i] = W_j . Vprev_i
        stale = np.zeros(k, dtype=bool)
        if not np.isfinite(np.diag(G)).all():
            if mutant is None:
                return np.full(W.shape, np.nan, np.float32), np.full(k, np.nan, np.float32), np.full(2, np.nan, np.float32)
            lam, E = np.full(k, np.nan), np.full((k, k), np.nan)        # what thirty Jacobi sweeps leave of a Gram matrix with one NaN
        else:
            lam, E = _eig_jacobi_like(0.5 * (G + G.T))
        order = rank_scatter(lam, total=mutant != "rank_plain") if np.isnan(lam).any() else np.argsort(-lam, kind="stable")
        stale = order == POISON
        order = np.where(stale, 0, order)
        lam, E = lam[order], E[:, order]
        lam[stale], E[:, stale] = STALE, STALE
        sig = np.sqrt(np.maximum(lam, 0.0) if mutant != "clamp" else np.where(lam > 0, lam, 0.0))      # np.maximum keeps a NaN
        dead = sig <= MIN_SIGMA if mutant != "clamp" else ~(sig > MIN_SIGMA)
        inv = np.where(dead, 0.0, 1.0 / np.where(dead, 1.0, sig))
        dot = np.einsum("ji,ji->i", E * inv[None, :], X)
        Cm = (np.where(dot < 0, -1.0, 1.0) * inv)[:, None] * E.T
        V = (Cm.astype(apply_dtype) @ W.astype(apply_dtype)).astype(np.float32)
        d = Vprev.astype(np.float32) - V
        d = np.where(np.isfinite(d), d, np.float32(np.nan))             # an inf difference (from Vprev) counts as NaN: conv is never inf
        conv0 = np.float32(np.sqrt((d.astype(np.float64) ** 2).sum()))
        viol = np.abs(d) - np.float32(1e-5) * np.abs(V)                 # fp32, as the kernel is written
        conv1 = np.float32(max_nan(np.float32(0), viol.max()) if mutant != "fmax" else max(np.float32(0), np.fmax.reduce(viol, axis=None)))
    return V, np.sqrt(sig).astype(np.float32), np.array([conv0, conv1], dtype=np.float32)


# ----------------------------------------------------------------------------------------------------------- non-finite input: cases and assertions
NF_K = [5, 6, 16, 17, 33, 57, 65, 97, 128]       # cyclic | round-robin 256 threads | <32> | <64> with apply<56> | tiled apply | <96> | eigenvectors in global memory
NF_N = 300                                       # ragged against the 256-column slices: two blocks, the second 44 columns
NF_SHAPES = [(k, NF_N) for k in NF_K] + [(128, 65795)]      # and the grid-stride route once
NF_VALUES = {"nan": np.nan, "pinf": np.inf, "ninf": -np.inf}
NF_POISONS = [f"{v}-{at}" for v in NF_VALUES for at in ("first", "tail")] + ["nan-row"]
NF_VPREV_K = [5, 40, 100]


def poisoned(A, how):
    """a copy of A [k][N] with one of NF_POISONS put in: `value-first` at [0][0], `value-tail` at [k-1][N-1], `nan-row` the whole row k // 2"""
    A = np.array(A, dtype=np.float32, copy=True)
    v, at = how.split("-")
    if at == "row":
        A[len(A) // 2, :] = np.nan
    else:
        A[(0, 0) if at == "first" else (len(A) - 1, A.shape[1] - 1)] = NF_VALUES[v]
    return A


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_all_nan(V, s, conv, what):
    """the rule for a non-finite W: every element of V, s and conv is NaN"""
    V, s, conv = np.asarray(V), np.asarray(s), np.asarray(conv)
    assert np.isnan(conv).all(), (what, "conv", conv)
    assert np.isnan(s).all(), (what, "s", s)
    assert np.isnan(V).all(), (what, "V", int(np.isnan(V).sum()), V.size)


def assert_vprev_rule(got, clean, what):
    """the rule for a finite W and a non-finite Vprev: s is bitwise the clean call's, |V| is bitwise the clean call's with one sign per row, conv is
    (NaN, NaN)"""
    (V, s, conv), (Vc, sc, _) = got, clean
    assert np.array_equal(_bits(s), _bits(sc)), (what, "s")
    assert np.array_equal(_bits(V) & 0x7FFFFFFF, _bits(Vc) & 0x7FFFFFFF), (what, "|V|")
    flipped = (_bits(V) != _bits(Vc))
    nz = (_bits(Vc) & 0x7FFFFFFF) != 0
    for i in range(len(V)):
        assert flipped[i][nz[i]].all() or not flipped[i][nz[i]].any(), (what, "row", i, "is neither the clean row nor its negative")
    assert np.isnan(np.asarray(conv)).all(), (what, "conv", conv)


# ----------------------------------------------------------------------------------------------------------- the kernel, called
def gpu_scratch(k, n, device="cuda:0"):
    """a scratch tensor for gpu_orth calls of shape (k, n), for the tests that reuse one across calls"""
    import torch

    from diffusion_pullback_amd import lib as L
    return torch.empty(int(L.load().dpb_orth_scratch_bytes(k, n)) // 8, dtype=torch.float64, device=device)


def gpu_orth(W, Vprev, inplace=False, device="cuda:0", scratch=None):
    """dpb_orth_checked on fp32 numpy (or device torch) inputs -> numpy (V, s, conv); inplace: V aliases Vprev; scratch: the caller's (gpu_scratch),
    default a fresh one"""
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
    if scratch is None:
        scratch = torch.empty(int(lib.dpb_orth_scratch_bytes(k, n)) // 8, dtype=torch.float64, device=device)
    assert scratch.numel() * 8 >= int(lib.dpb_orth_scratch_bytes(k, n)) and scratch.dtype == torch.float64
    L.check(lib.dpb_orth_checked(Wd.data_ptr(), Vpd.data_ptr(), V.data_ptr(), s.data_ptr(), conv.data_ptr(), scratch.data_ptr(), scratch.numel() * 8,
                                 k, n, C.c_void_p(torch.cuda.current_stream(device).cuda_stream)))
    torch.cuda.synchronize(device)
    return V.cpu().numpy(), s.cpu().numpy(), conv.cpu().numpy()
