#!/usr/bin/env python3
"""Time of the mesh voxeliser (dpc.render.meshvoxels, csrc/dpc_mesh_voxels.hip), stage by stage.

There is no ShapeNet on the machines this runs on, so the meshes are synthetic: --models meshes, alternately an icosphere
of 20 480 faces (thousands of sub-voxel faces) and a box of 12 faces that span the grid, at 32^3, 64^3 and 128^3, with each
fill.  Per grid and fill: the wall time of voxelise_meshes (packing and upload included), of the native call alone on
packed device buffers, and the kernels' own times from the library's launch record, against

    torch   the same rules composed from torch ops on the device: every (face, candidate node) pair expanded with
            repeat_interleave, the 13 axes evaluated elementwise in fp64 in the oracle's order, index_put_ into a bool grid;
            cummax-style prefix ORs for "carve"; (face, column) pairs, index_put_ with accumulate and a cumsum for "parity";
            --torch-chunk meshes at a time (the pair arrays are the memory bound)
    numpy   the oracle of tests/mesh_voxels_oracle.py on the host, for --host-items meshes (one of each kind), scaled

The native grids are asserted equal to the oracle's for the --host-items meshes, and compared with the torch composition's
(the count of differing voxels is recorded, 0 expected) before anything is timed.  Per kernel: the bytes it must move,
from the shapes, over its time, as a share of the HBM peak (8.0 TB/s) -- the kernels are bound by fp64 arithmetic and
LDS atomics, not by memory, and the shares say so.  One JSON line per (grid, fill), appended to
profiles/mesh_voxels_bench.jsonl (--out).

    python tools/bench_mesh_voxels.py [--models 256] [--reps 10] [--host-items 2] [--grids 32 64 128] [--out FILE]
    python tools/bench_mesh_voxels.py --once                   (every native stage once: for a kernel trace)
    python tools/bench_mesh_voxels.py --resource-usage [FILE]  (no device: the compiler's per-kernel resource usage)

Times are medians of --reps calls after a warm-up call, each call ended by a device synchronise."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib as BL
import numpy as np


def resource_usage(path):
    BL.resource_usage("dpc_mesh_voxels.hip", path, [
        "# k_mv_surface<fp64 input, words per workgroup, threads>, k_mv_parity<fp64 input, threads>, k_mv_carve<threads>; lds= is",
        "# the static part, all LDS is dynamic: k_mv_surface 4 bytes per word + 32 + 8 per thread (6176, 36896, 69664 B);",
        "# k_mv_carve 4 (2 (zs + halo) + 2) PW and k_mv_parity 4 ((zs + halo + 2) PW + threads + 2 + threads / 64 + 1) for",
        "# zs + halo planes of PW = H ceil(W / 32) words: at most 65536 B and 38988 B"])


def kernel_ms(fn, dev):
    fn()
    return BL.kernel_ms(fn, dev, "k_mv_")


def share(nbytes, ms):
    return BL.share(nbytes, ms, BL.HBM_PEAK, 5)


# --- the same rules from torch ops ---------------------------------------------------------------------------------
def _expand(counts):
    """(owner, local index) of sum(counts) items, counts[i] of them owned by i."""
    import torch

    owner = torch.repeat_interleave(torch.arange(len(counts), device=counts.device), counts)
    start = torch.cumsum(counts, 0) - counts
    return owner, torch.arange(len(owner), device=counts.device) - start[owner]


def _ranges(lo, hi, G):
    import torch

    a, b = torch.clamp(lo, min=0.0), torch.clamp(hi, max=float(G - 1))
    ok = a <= b
    return torch.where(ok, a, torch.zeros_like(a)).long(), torch.where(ok, b - a + 1, torch.zeros_like(a)).long()


def torch_surface(u, mesh_of, M, shape):
    """u [f,3,3] grid coordinates of the faces, mesh_of [f] -> bool [M,D,H,W]: the 13 axes on every candidate pair."""
    import torch

    D, H, W = shape
    a, n = [], []
    for c, G in enumerate(shape):
        ac, nc = _ranges(torch.ceil(u[:, :, c].amin(1) - 0.5), torch.floor(u[:, :, c].amax(1) + 0.5), G)
        a.append(ac)
        n.append(nc)
    face, loc = _expand(n[0] * n[1] * n[2])
    n1, n2 = n[1][face], n[2][face]
    node = [a[0][face] + loc // (n1 * n2), a[1][face] + (loc // n2) % n1, a[2][face] + loc % n2]
    uf = u[face]
    p = [[uf[:, v, c] - node[c].double() for c in range(3)] for v in range(3)]
    e = [[uf[:, 1, c] - uf[:, 0, c] for c in range(3)], [uf[:, 2, c] - uf[:, 1, c] for c in range(3)], [uf[:, 0, c] - uf[:, 2, c] for c in range(3)]]
    nr = [e[0][1] * e[1][2] - e[0][2] * e[1][1], e[0][2] * e[1][0] - e[0][0] * e[1][2], e[0][0] * e[1][1] - e[0][1] * e[1][0]]
    mn = lambda x, y, z: torch.minimum(torch.minimum(x, y), z)
    mx = lambda x, y, z: torch.maximum(torch.maximum(x, y), z)
    sep = torch.zeros(len(face), dtype=torch.bool, device=u.device)
    for c in range(3):
        sep |= (mn(p[0][c], p[1][c], p[2][c]) > 0.5) | (mx(p[0][c], p[1][c], p[2][c]) < -0.5)
    d = (nr[0] * p[0][0] + nr[1] * p[0][1]) + nr[2] * p[0][2]
    rad = 0.5 * ((nr[0].abs() + nr[1].abs()) + nr[2].abs())
    sep |= (d > rad) | (d < -rad)
    for k in range(3):
        i, j = (k + 1) % 3, (k + 2) % 3
        for ed in e:
            q = [ed[i] * p[v][j] - ed[j] * p[v][i] for v in range(3)]
            rad = 0.5 * (ed[i].abs() + ed[j].abs())
            sep |= (mn(*q) > rad) | (mx(*q) < -rad)
    keep = ~sep
    flat = ((mesh_of[face] * D + node[0]) * H + node[1]) * W + node[2]
    grid = torch.zeros(M * D * H * W, dtype=torch.bool, device=u.device)
    grid.index_put_((flat[keep],), torch.ones((), dtype=torch.bool, device=u.device))
    return grid.view(M, D, H, W)


def torch_carve(g):
    import torch

    out = torch.ones_like(g)
    b = g.to(torch.uint8)
    for ax in (1, 2, 3):
        out &= (torch.cummax(b, ax).values > 0) & (torch.flip(torch.cummax(torch.flip(b, [ax]), ax).values, [ax]) > 0)
    return out


def _edge(P, Q, cy, cx):
    import torch

    swap = (P[0] > Q[0]) | ((P[0] == Q[0]) & (P[1] > Q[1]))
    A = [torch.where(swap, Q[k], P[k]) for k in range(2)]
    B = [torch.where(swap, P[k], Q[k]) for k in range(2)]
    val = (B[1] - A[1]) * (cy - A[0]) - (B[0] - A[0]) * (cx - A[1])
    return torch.where(swap, -val, val)


def torch_parity(u, mesh_of, M, shape):
    """-> (bool [M,D,H,W] prefix XOR of the toggles, open columns [M])."""
    import torch

    D, H, W = shape
    P = [(u[:, v, 1], u[:, v, 2]) for v in range(3)]
    area = _edge(P[0], P[1], P[2][0], P[2][1])
    ya, ny = _ranges(torch.ceil(u[:, :, 1].amin(1)), torch.floor(u[:, :, 1].amax(1)), H)
    xa, nx = _ranges(torch.ceil(u[:, :, 2].amin(1)), torch.floor(u[:, :, 2].amax(1)), W)
    face, loc = _expand(torch.where(area != 0, ny * nx, torch.zeros_like(ny)))
    y, x = ya[face] + loc // nx[face], xa[face] + loc % nx[face]
    cy, cx = y.double(), x.double()
    neg = (area < 0)[face]
    inside = torch.ones(len(face), dtype=torch.bool, device=u.device)
    w = []
    for a_, b_ in ((1, 2), (2, 0), (0, 1)):
        Pa, Pb = (P[a_][0][face], P[a_][1][face]), (P[b_][0][face], P[b_][1][face])
        val = _edge(Pa, Pb, cy, cx)
        dy, dx = Pb[0] - Pa[0], Pb[1] - Pa[1]
        val, dy, dx = torch.where(neg, -val, val), torch.where(neg, -dy, dy), torch.where(neg, -dx, dx)
        inside &= (val > 0) | ((val == 0) & ((dy > 0) | ((dy == 0) & (dx < 0))))
        w.append(val)
    total = (w[0] + w[1]) + w[2]
    inside &= total != 0
    zs = ((w[0] * u[face, 0, 0] + w[1] * u[face, 1, 0]) + w[2] * u[face, 2, 0]) / total
    k = torch.clamp(torch.ceil(zs), 0.0, float(D))
    k = torch.where(inside, k, torch.zeros_like(k)).long()
    flat = ((mesh_of[face] * (D + 1) + k) * H + y) * W + x
    toggles = torch.zeros(M * (D + 1) * H * W, dtype=torch.int32, device=u.device)
    toggles.index_put_((flat[inside],), torch.ones((), dtype=torch.int32, device=u.device), accumulate=True)
    toggles = toggles.view(M, D + 1, H, W)
    return (torch.cumsum(toggles[:, :D], 1) & 1).bool(), (toggles.sum(1) & 1).sum((1, 2))


def torch_voxelise(verts, faces, desc, shape, fill, chunk):
    """The whole call from torch ops, `chunk` meshes at a time: (bool [M,D,H,W], open columns [M])."""
    import torch

    g1 = torch.tensor([s - 1 for s in shape], dtype=torch.float64, device=verts.device)
    grids, opened = [], []
    for a in range(0, len(desc), chunk):
        rows = desc[a:a + chunk]
        m = len(rows)
        f0, f1 = int(rows[0, 2]), int(rows[-1, 2] + rows[-1, 3])
        counts = torch.from_numpy(rows[:, 3].astype(np.int64)).to(verts.device)
        mesh_of = torch.repeat_interleave(torch.arange(m, device=verts.device), counts)
        vstart = torch.from_numpy(rows[:, 0].astype(np.int64)).to(verts.device)
        idx = faces[f0:f1].long() + vstart[mesh_of][:, None]
        u = (verts[idx].double() + 0.5) * g1
        s = torch_surface(u, mesh_of, m, shape)
        o = torch.zeros(m, dtype=torch.int64, device=verts.device)
        if fill == "carve":
            s = torch_carve(s)
        elif fill == "parity":
            par, o = torch_parity(u, mesh_of, m, shape)
            s = s | par
        grids.append(s)
        opened.append(o)
    return torch.cat(grids), torch.cat(opened)


# --- the workload ----------------------------------------------------------------------------------------------------
def workload(M, O):
    """M meshes, alternately an icosphere of 20 480 faces and a box of 12 grid-spanning faces, each a little different."""
    rng = np.random.default_rng(1)
    V5, F5 = O.icosphere(5, 1.0, dtype=np.float64)
    out = []
    for m in range(M):
        if m % 2 == 0:
            out.append(((V5 * (0.36 + 0.08 * rng.random()) + (rng.random(3) - 0.5) * 0.08).astype(np.float32), F5))
        else:
            lo, hi = -0.5 + 0.04 * rng.random(3), 0.5 - 0.04 * rng.random(3)
            V, F = O.box(lo, hi, np.float32)
            out.append((V, F))
    return out


_oracle_parts = {}


def oracle(O, mesh, shape, fill, key):
    """(grid, info) of the numpy oracle; the surface and the parity of a (grid, mesh) are computed once for the three fills."""
    if key not in _oracle_parts:
        s, _, outside = O.surface(mesh[0], mesh[1], shape)
        _oracle_parts[key] = (s, outside) + O.parity(mesh[0], mesh[1], shape)
    s, outside, par, opened = _oracle_parts[key]
    if fill == "none":
        return s, np.array([outside, 0])
    return (O.carve(s), np.array([outside, 0])) if fill == "carve" else (s | par, np.array([outside, opened]))


def bench_grid(a, G, fill, meshes, torch, R, O, dev):
    from dpc.render import _native
    from dpc.render import meshvoxels as MV

    shape = (G, G, G)
    M = len(meshes)
    code = MV.FILLS[fill]
    items, desc = MV._checked_meshes(meshes, shape, code, "bench")
    verts = torch.from_numpy(np.concatenate([V for V, _ in meshes])).to(dev)
    faces = torch.from_numpy(np.concatenate([F for _, F in meshes]).astype(np.int32)).to(dev)
    words = (G ** 3 + 31) // 32
    desc_d = torch.from_numpy(desc).to(dev)
    bits = torch.empty((M, words), dtype=torch.int32, device=dev)
    scratch, info = torch.empty_like(bits), torch.zeros((M, 2), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def native_call():
        rc = _native.lib().dpc_voxelise_meshes(_native.ptr(verts), int(verts.shape[0]), 0, _native.ptr(faces), int(faces.shape[0]),
                                               _native.ptr(desc_d), desc.ctypes.data_as(__import__("ctypes").c_void_p), M, G, G, G, code,
                                               _native.ptr(bits), _native.ptr(scratch), _native.ptr(info), _native.ptr(status),
                                               _native.stream_ptr(dev))
        _native.check(rc, "dpc_voxelise_meshes")

    grids, ginfo = R.voxelise_meshes(meshes, G, fill=fill, return_info=True)
    native_call()
    assert torch.equal(MV._unpack(bits, shape), grids) and torch.equal(info, ginfo) and int(status.item()) == 0
    if a.once:
        return None
    k = min(a.host_items, M)
    t0 = time.perf_counter()
    for m in range(k):
        ref, rinfo = oracle(O, meshes[m], shape, fill, (G, m))
        assert (grids[m].cpu().numpy() == ref).all() and ginfo[m].cpu().tolist() == rinfo.tolist(), (G, fill, m)
    host_ms = (time.perf_counter() - t0) * 1e3 / max(k, 1)     # the first fill of a grid pays for the surface and the parity
    tg, topen = torch_voxelise(verts, faces, desc, shape, fill, a.torch_chunk)
    differs = int((tg != grids).sum()) + int((topen != ginfo[:, 1]).sum())
    del tg
    t = BL.alternate({"native_wall": lambda: R.voxelise_meshes(meshes, G, fill=fill), "native_call": native_call,
                   "torch": lambda: torch_voxelise(verts, faces, desc, shape, fill, a.torch_chunk)}, a.reps)
    km = kernel_ms(native_call, dev)
    n_faces, n_verts = int(faces.shape[0]), int(verts.shape[0])
    slabs = -(-words // 16384) if words > 8192 else 1
    mesh_bytes = n_faces * 12 + n_verts * 12                      # a slab's workgroup reads its mesh once
    nbytes = {"k_mv_surface": mesh_bytes * slabs + M * words * 4}
    if fill == "carve":
        pw = G * ((G + 31) // 32)
        cslabs = -(-G // max(1, min(G, 7680 // pw)))
        nbytes["k_mv_carve"] = M * words * 4 * (cslabs + 1)       # every slab reads the whole grid, and writes its share
    if fill == "parity":
        pw = G * ((G + 31) // 32)
        cslabs = -(-G // max(1, min(G, 7680 // pw)))
        nbytes["k_mv_parity"] = mesh_bytes * cslabs + 2 * M * words * 4
    return {
        "bench": "mesh_voxels", "grid": G, "fill": fill, "meshes": M, "faces": n_faces, "vertices": n_verts, "reps": a.reps,
        "ms_median_min_max": t, "kernel_ms": km,
        "ratio_torch_over_native_call": round(t["torch"][0] / t["native_call"][0], 2),
        "ratio_torch_over_native_wall": round(t["torch"][0] / t["native_wall"][0], 2),
        "torch_chunk": a.torch_chunk, "voxels_torch_differs_in": differs,
        "kernel_bytes": nbytes, "kernel_share_of_hbm_peak": {k_: share(b, km.get(k_)) for k_, b in nbytes.items()},
        "numpy_meshes_timed": k, "numpy_host_ms_per_mesh": round(host_ms, 1), "numpy_host_ms_scaled_to_batch": round(host_ms * M, 1),
        "occupancy": round(float(grids.float().mean()), 4), "open_columns": int(ginfo[:, 1].sum()), "device": torch.cuda.get_device_name(0),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-items", type=int, default=2)
    ap.add_argument("--torch-chunk", type=int, default=8)
    ap.add_argument("--grids", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--fills", nargs="+", default=["none", "carve", "parity"])
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join(BL.ROOT, "profiles", "mesh_voxels_bench.jsonl"))
    ap.add_argument("--resource-usage", nargs="?", const=os.path.join(BL.ROOT, "profiles", "mesh_voxels_resource_usage.txt"))
    a = ap.parse_args()
    if a.resource_usage:
        resource_usage(a.resource_usage)
        return
    import torch

    import dpc.render as R
    import mesh_voxels_oracle as O

    dev = torch.device("cuda")
    meshes = workload(a.models, O)
    for G in a.grids:
        for fill in a.fills:
            res = bench_grid(a, G, fill, meshes, torch, R, O, dev)
            if res is not None:
                BL.emit(res, a.out)


if __name__ == "__main__":
    main()
