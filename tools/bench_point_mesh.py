#!/usr/bin/env python3
"""Time of the exact point-to-mesh distance (dpc.render.pointmesh, csrc/dpc_point_mesh.hip).

There is no ShapeNet on the machines this runs on, so the meshes are synthetic: icospheres and soups of small triangles
(tests/mesh_voxels_oracle.py) of about 1 k, 20 k and 100 k faces, one per model, each a little different; the points are
uniform in the cube.  Per (kind, faces):

    batch   --models models x --views views x --points points against the model's mesh, all rows in one call
    single  one view of one model alone: 32 point blocks, so the face range is split over workgroups

each with the wall time of point_mesh_distance (packing and upload included), of the native call alone on packed device
buffers, and k_pm_dist's own time from the library's launch record; point-face tests per second over the kernel time, and
the share of the fp64 vector peak (78.6 TFLOP/s, the data sheet's) at FLOPS_PER_TEST operations per test -- counted from
pm_d2 in csrc/dpc_point_mesh.hip: 25 fma, 14 mul, 7 add / sub, 9 min / max (the three clamps are two each, the running
minimum one), an fma as two; compares and selects are not counted.  Against

    torch   the same rule (the kernel's formulation) composed from torch ops on the device in fp64, the (point, face)
            pairs expanded by broadcasting, --torch-pairs pairs at a time, for --torch-models models of the batch; its time
            per test is what the ratio compares

The native distances of those models are compared with the torch composition's before anything is timed (the largest
difference in units of 2^-52 S^2 is recorded).  One JSON line per (kind, faces), appended to
profiles/point_mesh_bench.jsonl (--out).

    python tools/bench_point_mesh.py [--models 256] [--views 5] [--points 8000] [--faces 1000 20000 100000] [--reps 3]
    python tools/bench_point_mesh.py --once                   (every workload once: for a kernel trace)
    python tools/bench_point_mesh.py --resource-usage [FILE]  (no device: the compiler's per-kernel resource usage)

Times are medians of --reps calls after a warm-up call, each call ended by a device synchronise."""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib as BL
import numpy as np

FLOPS_PER_TEST = 80      # 25 fma x 2 + 14 mul + 7 add / sub + 9 min / max (csrc/dpc_point_mesh.hip: pm_d2 and the running min)


def resource_usage(path):
    BL.resource_usage("dpc_point_mesh.hip", path, [
        "# k_pm_dist<fp64 points, fp64 vertices>: lds= is the face tile, DPC_PM_FACE_TILE records of 12 double2 (static)"])


_base = {}


def mesh(kind, faces, seed):
    """(V fp32 [n,3], F int32 [f,3]): a soup of `faces` small triangles, or the icosphere whose face count 20 * 4^s is
    nearest to `faces` (in the logarithm); one base mesh per (kind, faces), scaled and moved a little by the seed."""
    import mesh_voxels_oracle as MV

    if (kind, faces) not in _base:
        if kind == "soup":
            _base[kind, faces] = MV.soup(faces, 1, dtype=np.float64)
        else:
            _base[kind, faces] = MV.icosphere(max(0, int(round(np.log(faces / 20.0) / np.log(4.0)))), 1.0)
    V, F = _base[kind, faces]
    rng = np.random.default_rng(seed)
    scale = (0.36 + 0.08 * rng.random()) if kind == "icosphere" else (0.9 + 0.1 * rng.random())
    return (V * scale + (rng.random(3) - 0.5) * 0.08).astype(np.float32), F


def torch_d2(P, tri, pairs):
    """Squared distances [n] of P [n,3] fp64 to the triangles tri [f,3,3] fp64 on the device: the kernel's rule from
    torch ops, at most `pairs` (point, face) pairs at a time."""
    import torch

    l = torch.stack([((tri[:, (k + 2) % 3] - tri[:, (k + 1) % 3]) ** 2).sum(1) for k in range(3)], 1)
    ia = torch.where((l[:, 0] >= l[:, 1]) & (l[:, 0] >= l[:, 2]), 0, torch.where(l[:, 1] >= l[:, 2], 1, 2))
    idx = torch.arange(len(tri), device=tri.device)
    A, B, C = tri[idx, ia], tri[idx, (ia + 1) % 3], tri[idx, (ia + 2) % 3]
    E0, E1, E2 = B - A, C - A, C - B
    dot = lambda x, y: x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1] + x[..., 2] * y[..., 2]
    a, b, c, e = dot(E0, E0), dot(E0, E1), dot(E1, E1), dot(E2, E2)
    N = torch.linalg.cross(E0, E1)
    nn = dot(N, N)
    area = nn > 0
    nan, zero = torch.full_like(nn, float("nan")), torch.zeros_like(nn)
    inv, ca, ba, aa = torch.where(area, 1 / nn, zero), torch.where(area, c / nn, nan), torch.where(area, b / nn, nan), torch.where(area, a / nn, nan)
    ia_, ic, ie = torch.where(a > 0, 1 / a, zero), torch.where(c > 0, 1 / c, zero), torch.where(e > 0, 1 / e, zero)
    out = torch.full((len(P),), float("inf"), dtype=torch.float64, device=P.device)
    fc = max(1, min(len(tri), pairs // max(1, min(len(P), 8192))))
    pc = max(1, pairs // fc)
    for p0 in range(0, len(P), pc):
        Pp = P[p0:p0 + pc, None, :]
        best = out[p0:p0 + pc]
        for f0 in range(0, len(tri), fc):
            s_ = slice(f0, f0 + fc)
            D = Pp - A[None, s_]
            d0, d1 = dot(D, E0[None, s_]), dot(D, E1[None, s_])
            s, t = ca[s_] * d0 - ba[s_] * d1, aa[s_] * d1 - ba[s_] * d0
            inside = (s >= 0) & (t >= 0) & (s + t <= 1)
            dn = dot(D, N[None, s_])
            plane = dn * dn * inv[s_]
            r = D - torch.clamp(d0 * ia_[s_], 0, 1)[..., None] * E0[None, s_]
            edge = dot(r, r)
            r = D - torch.clamp(d1 * ic[s_], 0, 1)[..., None] * E1[None, s_]
            edge = torch.minimum(edge, dot(r, r))
            G = D - E0[None, s_]
            r = G - torch.clamp(dot(G, E2[None, s_]) * ie[s_], 0, 1)[..., None] * E2[None, s_]
            edge = torch.minimum(edge, dot(r, r))
            best = torch.minimum(best, torch.where(inside, plane, edge).min(1).values)
        out[p0:p0 + pc] = best
    return out


def measure(clouds, meshes, mesh_of, reps, once, torch, dev):
    """Times of one workload: wall, native call, kernel; and the packed buffers' native result."""
    from dpc.render import _batch, _native, pointmesh

    plan = pointmesh._Plan(clouds, meshes, mesh_of, "bench")
    n_pts, n_verts, n_faces = plan.sizes
    pts, _ = _batch.pack(plan.clouds, dev, torch.float32)
    verts, _ = _batch.pack([V for V, _ in plan.items], dev, torch.float32)
    faces = torch.from_numpy(np.concatenate([F for _, F in plan.items])).to(dev)
    desc_d = torch.from_numpy(plan.desc).to(dev)
    L = _native.lib()
    ws = _batch.workspace(L.dpc_point_mesh_workspace_bytes(len(plan.desc)), dev)
    d2 = torch.empty((n_pts,), dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def native_call():
        rc = L.dpc_point_mesh_distance(_native.ptr(pts), n_pts, 0, _native.ptr(verts), n_verts, 0, _native.ptr(faces), n_faces,
                                       _native.ptr(desc_d), plan.desc.ctypes.data_as(ctypes.c_void_p), len(plan.desc), _native.ptr(d2),
                                       _native.ptr(ws), _native.ptr(status), _native.stream_ptr(dev))
        _native.check(rc, "dpc_point_mesh_distance")

    native_call()
    assert int(status.item()) == 0
    tests = int(sum(int(r[1]) * int(r[5]) for r in plan.desc))
    if once:
        return {"tests": tests}, d2
    wall = BL.median_ms(lambda: pointmesh.point_mesh_distance(clouds, meshes, mesh_of, squared=True), reps)
    call = BL.median_ms(native_call, reps)
    k_ms = BL.kernel_ms(native_call, dev, "k_pm_")
    dist_s = k_ms["k_pm_dist"] * 1e-3
    return {"tests": tests, "rows": len(plan.desc), "wall_ms_median_min_max": wall, "native_call_ms_median_min_max": call,
            "kernel_ms": k_ms, "tests_per_s": round(tests / dist_s, 1),
            "share_of_fp64_vector_peak": BL.share(tests * FLOPS_PER_TEST, k_ms["k_pm_dist"], BL.FP64_VECTOR_PEAK, 4)}, d2


def bench(a, kind, faces, torch, dev):
    rng = np.random.default_rng(5)
    meshes = [mesh(kind, faces, 100 + m) for m in range(a.models)]
    pts = (rng.random((a.models * a.views, a.points, 3)) - 0.5).astype(np.float32)
    mesh_of = [m for m in range(a.models) for _ in range(a.views)]
    batch, d2 = measure(list(pts), meshes, mesh_of, a.reps, a.once, torch, dev)
    single, d2_single = measure([pts[0]], meshes[:1], [0], a.reps, a.once, torch, dev)
    assert torch.equal(d2_single, d2[:a.points])              # split or not, the same bits
    if a.once:
        return None
    k = min(a.torch_models, a.models)
    P = torch.from_numpy(pts[:k * a.views]).to(dev).double()
    tris = [torch.from_numpy(V[F.astype(np.int64)]).to(dev).double() for V, F in meshes[:k]]
    run = lambda: torch.cat([torch_d2(P[m * a.views:(m + 1) * a.views].reshape(-1, 3), tris[m], a.torch_pairs) for m in range(k)])
    ref = run()
    got = d2[:k * a.views * a.points]
    S = max(float(pts[:k * a.views].__abs__().max()), max(float(np.abs(V).max()) for V, _ in meshes[:k]))
    differs = float((got - ref).abs().max()) / (2.0 ** -52 * S * S)
    t_ms = BL.median_ms(run, max(1, a.reps // 2))
    torch_tests = k * a.views * a.points * len(meshes[0][1])
    torch_ns = t_ms[0] * 1e6 / torch_tests
    native_ns = batch["native_call_ms_median_min_max"][0] * 1e6 / batch["tests"]
    return {"bench": "point_mesh", "kind": kind, "faces_per_mesh": len(meshes[0][1]), "models": a.models, "views": a.views,
            "points": a.points, "reps": a.reps, "flops_per_test": FLOPS_PER_TEST, "fp64_vector_peak_flops": BL.FP64_VECTOR_PEAK,
            "batch": batch, "single_view": single, "torch_models": k, "torch_pairs_per_chunk": a.torch_pairs,
            "torch_ms_median_min_max": t_ms, "torch_ns_per_test": round(torch_ns, 5), "native_call_ns_per_test": round(native_ns, 6),
            "ratio_torch_over_native_per_test": round(torch_ns / native_ns, 1), "max_difference_from_torch_in_units": round(differs, 3),
            "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", type=int, default=256)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--points", type=int, default=8000)
    ap.add_argument("--faces", type=int, nargs="+", default=[1000, 20000, 100000])
    ap.add_argument("--kinds", nargs="+", default=["icosphere", "soup"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--torch-models", type=int, default=1)
    ap.add_argument("--torch-pairs", type=int, default=1 << 24)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join(BL.ROOT, "profiles", "point_mesh_bench.jsonl"))
    ap.add_argument("--resource-usage", nargs="?", const=os.path.join(BL.ROOT, "profiles", "point_mesh_resource_usage.txt"))
    a = ap.parse_args()
    if a.resource_usage:
        resource_usage(a.resource_usage)
        return
    import torch

    dev = torch.device("cuda")
    for kind in a.kinds:
        for faces in a.faces:
            res = bench(a, kind, faces, torch, dev)
            if res is not None:
                BL.emit(res, a.out)


if __name__ == "__main__":
    main()
