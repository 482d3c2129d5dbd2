"""Numpy restatement of farthest-point sampling as include/dpc_render.h (dpc_fps) defines it, in fp64, one cloud at a time.

    d2(i,j) = (xi-xj)*(xi-xj) + (yi-yj)*(yi-yj) + (zi-zj)*(zi-zj), the additions left to right, nothing fused;
    dist = +inf everywhere, cur = first; per round: record cur and dist[cur], take cur, lower dist of every point not
    taken to min(dist, d2(., cur)), and move to the point not taken with the largest dist, ties to the lowest index.

A round is vectorised over the cloud; taken points carry dist = -1 for the arg-max (np.argmax returns the first maximum,
which is the tie rule).  brute_force is an independent O(n^2 m) statement of the same greedy rule used to check this
file; clouds() makes the seeded inputs the host and GPU tests share.
"""
import numpy as np


def d2_to(P, j):
    """Squared distances of every point of P (fp64 [n,3]) to point j, with the header's operation order."""
    dx, dy, dz = P[:, 0] - P[j, 0], P[:, 1] - P[j, 1], P[:, 2] - P[j, 2]
    return (dx * dx + dy * dy) + dz * dz


def fps(P, samples, first=0):
    """(indices int32 [samples], radius2 float64 [samples]) of the cloud P ([n,3], any float dtype: widened exactly)."""
    P = np.asarray(P).astype(np.float64)
    n = len(P)
    assert 1 <= samples <= n and 0 <= first < n
    dist = np.full(n, np.inf)
    taken = np.zeros(n, dtype=bool)
    idx = np.empty(samples, dtype=np.int32)
    rad = np.empty(samples, dtype=np.float64)
    cur = int(first)
    with np.errstate(over="ignore"):
        for k in range(samples):
            idx[k], rad[k] = cur, dist[cur]
            taken[cur] = True
            dist = np.where(taken, dist, np.minimum(dist, d2_to(P, cur)))
            cur = int(np.argmax(np.where(taken, -1.0, dist)))
    return idx, rad


def brute_force(P, samples, first=0):
    """The same greedy rule from the full distance matrix, with plain Python loops: (indices, radius2)."""
    P = np.asarray(P).astype(np.float64)
    n = len(P)
    D = np.array([[((P[i, 0] - P[j, 0]) * (P[i, 0] - P[j, 0]) + (P[i, 1] - P[j, 1]) * (P[i, 1] - P[j, 1]))
                   + (P[i, 2] - P[j, 2]) * (P[i, 2] - P[j, 2]) for j in range(n)] for i in range(n)]).reshape(n, n)
    picks, rad = [int(first)], [np.inf]
    while len(picks) < samples:
        best, arg = -1.0, -1
        for i in range(n):
            if i in picks:
                continue
            r = min(D[i, j] for j in picks)
            if r > best:   # strict: the lowest index of a tie stays
                best, arg = r, i
        picks.append(arg)
        rad.append(best)
    return np.array(picks, dtype=np.int32), np.array(rad)


def clouds(kind, n, seed, dtype=np.float64):
    """A seeded cloud [n,3]: "random" is uniform in the unit cube around 0; "lattice" has integer coordinates in [0, 4)
    (64 distinct points: many exact ties, and coincident points once n > 64)."""
    rng = np.random.default_rng(seed)
    if kind == "lattice":
        return rng.integers(0, 4, size=(n, 3)).astype(dtype)
    return (rng.random((n, 3)) - 0.5).astype(dtype)
