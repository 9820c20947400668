"""Numpy float64 restatement of flag k-means (geometry.flag_kmeans) and of the chordal affinity of subspaces of unequal rank, in the AMBIENT space on
purpose: every member is orthonormalised by QR, a cluster's centre is ``flag_mean_ref`` of its members (one SVD of the stacked Q's), the affinity is
``||Q Y^T||_F^2`` -- none of the Gram / coefficient algebra of csrc/flagkmeans.hip.  Also the planted sets of the tests and the trajectory cases."""
import numpy as np

import _flag_ref as FR
from _frechet_ref import mixing, orthonormal_rows, random_orthonormal

MOVE_MARGIN = 1e-12                  # a member moves only if the best affinity exceeds its own by more than this times r


def affinity_ref(a, y):
    """a [B, k, N], y [C, r, N] (rows independent, any scale) -> aff [B, C] float64 = ||Q_a Q_y^T||_F^2 = sum cos^2 of the principal angles"""
    qa = [orthonormal_rows(x) for x in np.asarray(a, np.float64)]
    qy = [orthonormal_rows(x) for x in np.asarray(y, np.float64)]
    return np.array([[np.sum((q @ c.T) ** 2) for c in qy] for q in qa])


def _affinity_q(qs, ys):
    return np.array([[np.sum((q @ y.T) ** 2) for y in ys] for q in qs])


def seeds_ref(qs, n_clusters, init=0):
    """the seed members and the start labels: farthest-first on D^2(i, s) = k - ||Q_i Q_s^T||_F^2 (lowest index on a tie) from member ``init``, or the
    given sequence; every member takes the nearest seed (lowest cluster on a tie), a seed its own cluster"""
    b, k = len(qs), qs[0].shape[0]
    d2 = lambda s: np.array([k - np.sum((q @ qs[s].T) ** 2) for q in qs])
    given = not isinstance(init, (int, np.integer))
    seeds = [int(s) for s in init] if given else [int(init)]
    dist = np.empty((n_clusters, b))
    dmin = np.full(b, np.inf)
    for t in range(n_clusters):
        if t >= len(seeds):
            seeds.append(int(np.argmax(dmin)))         # (argmax returns the lowest index of the largest)
        dist[t] = d2(seeds[t])
        dmin = np.minimum(dmin, dist[t])
        dmin[seeds[:t + 1]] = -np.inf                   # a seed leaves the race
    labels = np.argmin(dist, axis=0)                    # (the lowest cluster on a tie)
    labels[seeds] = np.arange(n_clusters)
    return seeds, labels.astype(np.int64)


def renumber(labels):
    """clusters renumbered by their lowest member index: (new labels, perm) with perm[new] = old"""
    first = {}
    for i, c in enumerate(labels):
        first.setdefault(int(c), i)
    perm = sorted(first, key=first.get)
    inv = {old: new for new, old in enumerate(perm)}
    return np.array([inv[int(c)] for c in labels]), perm


def flag_kmeans_ref(a, n_clusters, rank=None, init=0, max_rounds=50):
    """a [B, k, N] -> (labels [B], Y [C, r, N] float64, info).  info: rounds, converged, objective (one entry per fit), moved, kept, sizes, weight [C, r],
    eigenvalues (per cluster, all of them), affinity [B, C], seeds, history (the labels after every round, in the run's own numbering), and per fit the
    smallest decision margin (own affinity against the best other; inf for C = 1) and the smallest relative gap after row r over the clusters."""
    a = np.asarray(a, np.float64)
    b, k, _ = a.shape
    r = k if rank is None else int(rank)
    qs = [orthonormal_rows(x) for x in a]
    seeds, labels = seeds_ref(qs, n_clusters, init)
    objective, moved, history, margins, gaps = [], [], [], [], []
    kept, rounds, converged = 0, 0, False
    while True:
        fits = [FR.flag_mean_ref(a[labels == c], r) for c in range(n_clusters)]
        ys = [f[0] for f in fits]
        aff = _affinity_q(qs, ys)
        own = aff[np.arange(b), labels]
        objective.append(float(np.sum(r - own)))
        other = aff.copy()
        other[np.arange(b), labels] = -np.inf
        margins.append(float(np.min(np.abs(own - other.max(axis=1)))) if n_clusters > 1 else float("inf"))
        gaps.append(min(float(FR.rel_gaps(f[1]["eigenvalues"])[r - 1]) for f in fits))
        if rounds == max_rounds:
            break
        best = np.argmax(aff, axis=1)                   # (the lowest c on a tie)
        want = np.where(aff[np.arange(b), best] > own + MOVE_MARGIN * r, best, labels)
        for c in range(n_clusters):
            mem = np.nonzero(labels == c)[0]
            if len(mem) and not np.any(want[mem] == c):
                want[mem[int(np.argmax(aff[mem, c]))]] = c
                kept += 1
        n = int(np.sum(want != labels))
        rounds += 1
        moved.append(n)
        if n == 0:
            converged = True
            break
        labels = want
        history.append(labels.copy())
    final, perm = renumber(labels)
    info = {"rounds": rounds, "converged": converged, "objective": np.array(objective), "moved": moved, "kept": kept,
            "sizes": np.bincount(final, minlength=n_clusters), "weight": np.stack([fits[c][1]["weight"] for c in perm]),
            "eigenvalues": [fits[c][1]["eigenvalues"] for c in perm], "affinity": aff[:, perm], "seeds": [seeds[c] for c in perm],
            "history": history, "margin": margins, "gap": gaps, "start": seeds_ref(qs, n_clusters, init)[1]}
    return final, np.stack([ys[c] for c in perm]), info


def planted_set(rng, sizes, k, n, r, noise, cond=10.0):
    """(a [B, k, N] float32, truth [B]): one family per entry of sizes, each with r shared directions of its own, perturbed per member by
    noise N(0, 1) / sqrt(N), plus k - r private random rows; rows mixed at condition cond; members shuffled"""
    out, truth = [], []
    for c, size in enumerate(sizes):
        shared = random_orthonormal(rng, r, n)
        for _ in range(size):
            rows = shared + noise * rng.standard_normal((r, n)) / np.sqrt(n)
            rows = np.concatenate([rows, rng.standard_normal((k - r, n)) / np.sqrt(n)])
            out.append(mixing(rng, k, cond) @ rows)
            truth.append(c)
    order = rng.permutation(len(out))
    return np.stack(out)[order].astype(np.float32), np.array(truth)[order]


def same_partition(x, y):
    return np.array_equal(renumber(np.asarray(x))[0], renumber(np.asarray(y))[0])


def seeds_inside(truth, family, n):
    """the n lowest member indices of one planted family: seeds that all sit in one cluster, so that rounds with moves are needed"""
    return [int(i) for i in np.nonzero(np.asarray(truth) == family)[0][:n]]


# the trajectory cases: (sizes, k, N, r, noise, rng seed): k no multiple of 4, k = 64, R_c no multiple of 16 or 32, R > N, unequal clusters.  Every seed
# sits inside planted family 0.  tests/test_flag_kmeans_host.py asserts on the CPU that in EVERY round of the reference the relative gap after row r is >= MIN_GAP in every cluster and every member's decision margin >= MIN_MARGIN
TRAJECTORY_CASES = (                          # moves per round, smallest margin, smallest gap of the reference
    ((4, 4, 4), 3, 24, 2, 0.5, 500),          # 2, 3, 0     0.022   0.155
    ((4, 4, 4), 3, 24, 2, 0.5, 501),          # 2, 2, 2, 0  0.0097  0.085
    ((6, 6), 5, 67, 3, 0.7, 502),             # 1, 5, 0     0.113   0.055
    ((7, 5, 4, 4), 6, 130, 2, 0.5, 501),      # 7, 2, 0     0.068   0.103
    ((10, 10, 10), 8, 260, 3, 0.6, 501),      # 10, 4, 0    0.017   0.196
    ((5, 5), 16, 517, 4, 0.6, 1),             # 4, 0        1.76    0.154
    ((4, 3), 64, 4099, 3, 0.6, 2),            # 2, 0        1.68    0.240
)
MIN_GAP, MIN_MARGIN = 0.05, 1e-3


def trajectory_case(case):
    sizes, k, n, r, noise, rng_seed = case
    a, truth = planted_set(np.random.default_rng(rng_seed), sizes, k, n, r, noise)
    return a, truth, seeds_inside(truth, 0, len(sizes)), r
