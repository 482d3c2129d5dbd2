#!/usr/bin/env python3
"""Training-view rendering with textures and smooth normals against the flat renderer, and the flat renderer against
another build of the library: bench_mesh_render's synthetic split (--models height-field meshes, 5 views each, S = 128,
ss = 3) with one uv and one normal per vertex and one procedural texture per model.  Appends one JSON line to --out and
prints it.

    python tools/bench_mesh_shaded.py [--models 64] [--views 5] [--faces 2000 20000 200000] [--texture-sizes 256 512 1024]
                                      [--image-size 128] [--supersample 3] [--reps 5] [--rounds 3] [--parent-lib PATH]
                                      [--out profiles/mesh_shaded_bench.jsonl]
    python tools/bench_mesh_shaded.py --child shaded          # one shaded measurement alone (for rocprofv3)

ASSUMED face counts and texture sizes: the models' face counts cycle through --faces and their square textures through
--texture-sizes (256, 512 and 1024 texels a side by default); neither has been measured on ShapeNet here.

Every measurement runs in a child process of its own, one at a time, each under its own time limit; a child that fails
ends the run.  flat: render_mesh_views on the plain scenes from host arrays to a device synchronise, after a warm-up, over
--reps repeats, and the library's own event timing of one call per kernel.  With --parent-lib (a build of the parent
commit, tools/build_variant.sh with SRC_REV) the flat child runs --rounds times with each build, alternating; the parent's
medians against each other give the run-to-run spread, and flat_passes says whether the median of this build's medians
is not above the parent's by more than that spread.  shaded: the same scenes as ShadedScenes, flat and shaded timed in one
process, the ratio, and the bytes the shading reads, from the shapes: 12 bytes of texels per covered sample (four RGB
texels), and per covered sample at most 172 bytes of attributes (three uvs and normals with their indices, the
material's texture and its row), less where neighbouring samples of a pixel share the face."""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib as BL


def arguments():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", type=int, default=64)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--faces", type=int, nargs="+", default=[2000, 20000, 200000])
    ap.add_argument("--texture-sizes", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--image-size", type=int, default=128)
    ap.add_argument("--supersample", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child", choices=["flat", "shaded"], default="")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(BL.ROOT, "profiles", "mesh_shaded_bench.jsonl"))
    return ap.parse_args()


def child(a):
    import numpy as np
    import torch

    from dpc.render import _native

    if a.child == "flat":   # a build of the parent commit lacks the shaded symbols; the flat child does not call them
        _native._FUNCTIONS = tuple(f for f in _native._FUNCTIONS if "meshes_shaded" not in f[0])
    import dpc.render as R
    import mesh_render_oracle as O
    import mesh_shade_oracle as SO

    n_of = lambda i: max(1, int(round((a.faces[i % len(a.faces)] / 2) ** 0.5)))
    side = lambda i: a.texture_sizes[i % len(a.texture_sizes)]
    kd = np.array([[0.3, 0.3, 0.9], [0.9, 0.9, 0.2]])
    plain = [O.grid_mesh(n_of(i), seed=i) + (kd,) for i in range(a.models)]
    pos = R.sample_camera_positions(a.models, a.views, 0)
    dev = torch.device("cuda")
    S, ss = a.image_size, a.supersample

    def measure(scenes):
        out = None

        def run():
            nonlocal out
            out = R.render_mesh_views(scenes, pos, image_size=S, supersample=ss)

        R.render_mesh_views(scenes[:2], pos[:2], image_size=32)   # warm-up: code object, allocator
        times = BL.walls_ms(run, a.reps)
        kernels = {k: float(np.sum(v)) for k, v in _native.profile_kernels(run, dev).items()}
        return dict(render_ms_median=float(np.median(times)), render_ms_min=min(times), render_ms_max=max(times),
                    kernel_ms=kernels), out

    res = dict(faces_total=int(sum(len(s[1]) for s in plain)), lib=os.environ.get("DPC_RENDER_LIB") or "in-tree",
               device=torch.cuda.get_device_name(dev))
    res["flat"], out = measure(plain)
    if a.child == "shaded":
        shaded = []
        for i in range(a.models):
            s = SO.shaded_grid(n_of(i), i, [SO.checker(side(i), side(i), i)], mat_tex=(0, 0), Kd=kd)
            shaded.append(R.ShadedScene(*s[:4], None, *s[4:], []))
        res["shaded"], out2 = measure(shaded)
        assert out2[1].cpu().numpy().tobytes() == out[1].cpu().numpy().tobytes()      # the same geometry
        covered = int(O.covered_from_alpha(out2[0][..., 3].cpu().numpy(), ss).sum())
        res.update(covered_samples=covered, texel_bytes_read=12 * covered, attribute_bytes_read_max=172 * covered,
                   texture_bytes_uploaded=int(sum(t.size for s in shaded for t in s.textures)),
                   wall_ratio=res["shaded"]["render_ms_median"] / res["flat"]["render_ms_median"],
                   tile_kernel_ratio=res["shaded"]["kernel_ms"]["k_mr_tile"] / res["flat"]["kernel_ms"]["k_mr_tile"])
    print("RESULT " + json.dumps(res))


def run_child(a, kind, lib):
    env = dict(os.environ)
    env.pop("DPC_RENDER_LIB", None)
    if lib:
        env["DPC_RENDER_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--models", str(a.models), "--views", str(a.views),
           "--image-size", str(a.image_size), "--supersample", str(a.supersample), "--reps", str(a.reps), "--faces"] + \
        [str(f) for f in a.faces] + ["--texture-sizes"] + [str(t) for t in a.texture_sizes]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
    lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        print(r.stdout[-2000:], r.stderr[-4000:])
        sys.exit("bench_mesh_shaded: the %s child (%s) failed with exit status %d; nothing more is started"
                 % (kind, lib or "in-tree", r.returncode))
    return json.loads(lines[0][7:])


def main():
    a = arguments()
    if a.child:
        return child(a)
    import numpy as np

    line = dict(tool="bench_mesh_shaded", models=a.models, views_per_model=a.views, faces_assumed=a.faces,
                texture_sizes_assumed=a.texture_sizes, image_size=a.image_size, supersample=a.supersample, reps=a.reps)
    if a.parent_lib:
        lib = os.path.abspath(a.parent_lib)
        rounds = {"this": [], "parent": []}
        for _ in range(a.rounds):
            rounds["this"].append(run_child(a, "flat", ""))
            rounds["parent"].append(run_child(a, "flat", lib))
        med = {k: [r["flat"]["render_ms_median"] for r in v] for k, v in rounds.items()}
        tile = {k: [r["flat"]["kernel_ms"]["k_mr_tile"] for r in v] for k, v in rounds.items()}
        spread = max(med["parent"]) - min(med["parent"])
        line["flat_ab"] = dict(rounds=a.rounds, this_medians_ms=med["this"], parent_medians_ms=med["parent"],
                               this_median_ms=float(np.median(med["this"])), parent_median_ms=float(np.median(med["parent"])),
                               parent_spread_ms=spread, this_tile_kernel_ms=tile["this"], parent_tile_kernel_ms=tile["parent"],
                               flat_passes=bool(np.median(med["this"]) <= np.median(med["parent"]) + spread))
    res = run_child(a, "shaded", "")
    line.update(res)
    BL.emit(line, a.out)


if __name__ == "__main__":
    main()
