"""The auction of csrc/dpc_emd.hip restated in numpy fp64, round for round (the contract is in include/dpc_render.h,
dpc_emd_fwd), and the inputs the EMD tests share.

    cost_matrix   c_ij = d2 or sqrt(d2), d2 = dx*dx + dy*dy + dz*dz added left to right
    auction       span = max c - min c; eps_0 = max(span / 2, eps), eps_k = max(eps_{k-1} / 5, eps), the last phase runs
                  with exactly eps; prices start at 0 and carry over, every phase starts with nobody assigned; Jacobi
                  rounds on one snapshot: v_ij = -c_ij - price_j, j* the first argmax, w the best of the rest (v when
                  n = 1), bid = price_j* + (v - w) + eps_k; an object goes to its highest bid, ties to the lowest bidder,
                  its price becomes the bid and its previous owner is unassigned; after max_rounds rounds in total a pair
                  with rounds still to run stops as not converged
    device_mean   the kernel's summation order for emd
    clouds        the random and lattice inputs by (kind, n, seed, dtype)
"""
import hashlib

import numpy as np


def cost_matrix(P, G, squared):
    P, G = np.asarray(P, dtype=np.float64), np.asarray(G, dtype=np.float64)
    dx = P[:, None, 0] - G[None, :, 0]
    dy = P[:, None, 1] - G[None, :, 1]
    dz = P[:, None, 2] - G[None, :, 2]
    d2 = dx * dx + dy * dy + dz * dz
    return d2 if squared else np.sqrt(d2)


def auction(C, eps, max_rounds=10 ** 9):
    """{"assignment": pi [n], "inverse": [n], "rounds": int, "converged": bool}; unassigned entries are -1."""
    C = np.asarray(C, dtype=np.float64)
    n = C.shape[0]
    eps = float(eps)
    price = np.zeros(n)
    span = C.max() - C.min()
    eps_k = max(span / 2, eps)
    rounds = 0
    assigned, owner = -np.ones(n, dtype=np.int64), -np.ones(n, dtype=np.int64)
    while True:
        assigned[:] = -1
        owner[:] = -1
        while (assigned < 0).any():
            if rounds >= max_rounds:
                return {"assignment": assigned, "inverse": owner, "rounds": rounds, "converged": False}
            rounds += 1
            un = np.flatnonzero(assigned < 0)
            rows = np.arange(len(un))
            V = -C[un] - price[None, :]
            j = V.argmax(axis=1)            # the first maximum: the lowest j
            v = V[rows, j]
            if n > 1:
                V[rows, j] = -np.inf
                w = V.max(axis=1)
            else:
                w = v
            bid = price[j] + (v - w) + eps_k
            order = np.lexsort((un, -bid, j))   # per object: the highest bid first, among equals the lowest bidder
            jj = j[order]
            win = order[np.r_[True, jj[1:] != jj[:-1]]]
            obj, who = j[win], un[win]
            old = owner[obj]
            assigned[old[old >= 0]] = -1
            owner[obj] = who
            assigned[who] = obj
            price[obj] = bid[win]
        if eps_k <= eps:
            return {"assignment": assigned, "inverse": owner, "rounds": rounds, "converged": True}
        eps_k = max(eps_k / 5, eps)


def device_mean(terms):
    """sum(terms) / n in the kernel's order: partial sum l adds terms l, l + 64, ... in ascending order onto 0.0, then a
    butterfly over the 64 partial sums at distances 32, 16, ... 1."""
    terms = np.asarray(terms, dtype=np.float64)
    part = np.zeros(64)
    for l in range(64):
        s = 0.0
        for x in terms[l::64]:
            s = s + x
        part[l] = s
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        part = part + part[lanes ^ off]
    return part[0] / np.float64(len(terms))


def emd(P, G, squared, eps, max_rounds=10 ** 9):
    """The oracle's whole answer for one pair: auction()'s dict plus "emd" (NaN when not converged) and "total"."""
    C = cost_matrix(P, G, squared)
    out = auction(C, eps, max_rounds)
    if out["converged"]:
        terms = C[np.arange(len(C)), out["assignment"]]
        out["emd"], out["total"] = device_mean(terms), terms.sum()
    else:
        out["emd"], out["total"] = np.nan, np.nan
    return out


def clouds(kind, n, seed, dtype=np.float64):
    """(pred, gt), each [n,3] in dtype.  "random": uniform in [-0.5, 0.5)^3.  "lattice": the same rounded to multiples of
    1/8, so squared distances are multiples of 1/64 with many exact ties and coincident points."""
    rng = np.random.default_rng(seed)
    P, G = rng.random((n, 3)) - 0.5, rng.random((n, 3)) - 0.5
    if kind == "lattice":
        P, G = np.round(P * 8) / 8, np.round(G * 8) / 8
    elif kind != "random":
        raise ValueError(kind)
    return P.astype(dtype), G.astype(dtype)


def checksum(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# The fixture's cases (tests/golden/make_golden_emd.py writes them, tests/test_emd_host.py and test_emd_gpu.py read them):
# (kind, n, dtype name, squared).  The seed of a case is its position in this list.
FIXTURE_CASES = ([("random", n, dt, sq) for n in (1, 2, 64, 257, 1000) for dt in ("float32", "float64") for sq in (True, False)]
                 + [("lattice", n, "float64", True) for n in (300, 1000)])


def case_key(kind, n, dt, squared):
    return "%s_n%d_%s_%s" % (kind, n, dt, "sq" if squared else "l2")
