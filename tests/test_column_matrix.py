"""Every instantiation of the loss columns against the oracle, once.

The expected-depth loss (csrc/dpc_depth.hip) and the ray-consistency mask loss (csrc/dpc_drc_loss.hip) are shells around one
skeleton (csrc/dpc_ray_column.h) that column_dispatch instantiates for the depths 32, 64, 128 and the nine tap buckets of
plan_taps, forward and backward: 27 x 2 compiled kernels per loss plus the two generic (`_dyn`) ones, each with its own
register window, unrolled D pass, adjoint D pass and launch bounds.  Each answers to the fp64 oracles here
(tests/depth_loss_oracle.py, tests/drc_loss_oracle.py), in the style of tests/test_kernel_matrix.py:

  - MATRIX is a declarative table, one row per (loss, D, bucket); a row names THE TWO INSTANTIATIONS IT MUST LAUNCH.  The GPU
    case calls the C ABI directly (outputs pre-filled with NaN, workspace with 0xA5 except the zeroed tickets), checks the
    launch record -- forward exactly [fwd id, k_tile_loss_finalize], backward exactly [bwd id] -- and compares loss, depth
    map, dgrid_wh and ds under the parity rule of tests/test_gpu_parity.py, max|dev - ref| <= 1e-5 * max(1, max|ref|).
  - The z kernels are `skewed` (test_kernel_matrix.py): positive, normalised and ASYMMETRIC, every tap far above plan_taps'
    drop threshold.  The backward uses the flipped taps (make_taps<RB>(.., true), resolve_taps(.., flip), the generic kernels'
    "taps read backwards"); test_rows_tell_a_flipped_kernel_apart shows on the oracle that flipping the kernel moves every
    row's loss and dgrid_wh by >= 100 parity bounds, so an adjoint that correlates where it should convolve cannot hide.
    Most rows fill the window (radius = bucket); rows of the buckets 6, 8, 10, 15 also run radius = bucket - 1 (the window's
    ends zero -- below bucket 6 the buckets are consecutive, a radius of bucket - 1 IS the next bucket); some rows hand over a
    21-tap array whose outer taps are exactly zero (make_taps' centring c = (taps - 1) / 2, unflipped and flipped).
  - GENERIC: asymmetric kernels on the generic kernels (another depth, a 33-tap kernel).  DEVICE: the z taps read from device
    memory (DpcParams.dev_taps_z, a DeviceSchedule's) -- the host array only picks the bucket, the device holds OTHER values
    and the oracle runs with those; test_device_rows_tell_the_host_taps_apart shows a kernel that ignored device memory would
    miss by >= 100 bounds.  ZERO_S: a cloud whose scale is 0 (ds takes the rc.s != 0 branch): its dgrid_wh and ds are exactly 0.
  - test_matrix_names_every_column_instantiation_in_the_build (CPU) reads the kernel symbols of dpc_depth.o, dpc_drc_loss.o
    and dpc_rgb.o: exactly the rows' ids plus ELSEWHERE.  A bucket added to or dropped from column_dispatch fails the CPU suite.

Inputs (B = 2: a non-zero buffer base per cloud; H = W = 18: 324 rays, the second ray tile has 68 live lanes, so the dead-lane
path and the two-tile ds hand-off run): a sparse grid of about four occupied voxels per ray, values 0.02 .. 1.1, whole empty
rays; scales divided by the kernel's largest tap, so that some s v exceed 1 at every radius.  The gradients are discontinuous
at the clamps: every row asserts on the oracle that no pre-clamp value lies within 1e-6 of eps, 1 - eps or 1, that s v > 1
somewhere (rows with s), max|dgrid_ref| > 1e-3, ds_ref != 0 and, for depth, depth_ref.min() < 0.9 max_depth.  The seeds are in
the table and were checked on the CPU (test_rows_meet_their_input_conditions); a row that fails gets another seed.

Why so many mask rows carry a seed and a salt of their own: dgrid_wh tells a flipped kernel apart by thousands of bounds on
every row, the VALUE of the mask loss hardly at all.  A ray's cost depends on the occupancies only through prod (1 - y_z), and
an isolated voxel smeared with the flipped kernel leaves the same values in mirrored order; what is left are the overlaps of
neighbouring smears and the tails cut off at the two ends of the ray, which differ from ray to ray in sign.  With the default
seed the loss moved by 2 .. 100 bounds; seed and salt were searched (40 seeds x 12 salts) until it moved by >= 100, and where
no pair did the row lost its scale s (a large s saturates the rays).  The depth loss weighs the voxels by their depth and has
no such symmetry.  The same holds for host against device taps, so some device kernels are a little narrower than the window."""
import ctypes
import os
import zlib
from collections import namedtuple

import numpy as np
import pytest
import torch

import depth_loss_oracle as DO
import drc_loss_oracle as DR
from test_depth_loss_gpu import e2e_inputs, launch_list
from test_gpu_parity import ERRORS, TOL, close
from test_kernel_matrix import BUCKETS, built_instantiations, skewed

B, G = 2, 18
DEPTHS = (32, 64, 128)
EPS, MARGIN = 1e-5, 1e-6
CAMERA, MAX_DEPTH, MAX_DATASET_DEPTH = 2.0, 7.5, 10.0     # the depth loss's; the mask loss reads neither depth
COLUMN_OBJECTS = ("dpc_depth.o", "dpc_drc_loss.o", "dpc_rgb.o")
FIN = "k_tile_loss_finalize"
SEPARATION = 100.0    # a flipped kernel / the host's taps must move the oracle by this many parity bounds

# Kernels of the three objects that other files pin: id -> (test file, the string that names it there).  The forward generic
# kernels are named there through their backward twin (c.kernel.replace("bwd", "fwd")); the colour projection's two kernels
# have one instantiation each and no launcher choice to pin: every case of the file launches them through proj_rgb_loss.
ELSEWHERE = {
    "k_depth_fwd_dyn": ("test_depth_loss_gpu.py", '"k_depth_bwd_dyn"'),
    "k_depth_bwd_dyn": ("test_depth_loss_gpu.py", '"k_depth_bwd_dyn"'),
    "k_drcmask_fwd_dyn": ("test_drc_loss_gpu.py", '"k_drcmask_bwd_dyn"'),
    "k_drcmask_bwd_dyn": ("test_drc_loss_gpu.py", '"k_drcmask_bwd_dyn"'),
    FIN: ("test_drc_loss_gpu.py", '"k_tile_loss_finalize"'),
    "k_drcrgb_fwd": ("test_drc_loss_gpu.py", '"k_drcrgb_fwd"'),
    "k_drcrgb_bwd<32>": ("test_drc_loss_gpu.py", '"k_drcrgb_bwd<32>"'),
    "k_drcrgb_bwd<64>": ("test_drc_loss_gpu.py", '"k_drcrgb_bwd<64>"'),
    "k_drcrgb_bwd_dyn": ("test_drc_loss_gpu.py", '"k_drcrgb_bwd_dyn"'),
    "k_rgb_fwd": ("test_rgb_loss_gpu.py", "R.proj_rgb_loss("),
    "k_rgb_bwd": ("test_rgb_loss_gpu.py", "R.proj_rgb_loss("),
}


def col(loss, D, rb):
    """(forward id, backward id) of a loss column; rb None: the generic kernels."""
    if rb is None:
        return ("k_%s_fwd_dyn" % loss, "k_%s_bwd_dyn" % loss)
    return ("k_%s_fwd<%d, %d>" % (loss, D, rb), "k_%s_bwd<%d, %d>" % (loss, D, rb))


def centred(core, n=None):
    """The taps `core` in the middle of an n-tap array of zeros (n None: as they are)."""
    core = np.asarray(core, dtype=np.float32)
    n = core.size if n is None else n
    out = np.zeros(n, dtype=np.float32)
    c, r = (n - 1) // 2, (core.size - 1) // 2
    out[c - r:c + r + 1] = core
    return out


# kz: the host taps (None: taps_z = 0, no D pass); dev: the values in device memory (None: no DpcParams.dev_taps_z); r: the
# effective radius of kz; flags: s / w / dloss / ddepth present; f: the ground truth is f times the map; zero_s: cloud 0 has s = 0
Row = namedtuple("Row", "name loss D rb r kz dev s w dloss ddepth f seed zero_s ids")


def row(loss, D, rb, flags="", r=None, n=None, salt=1.9, seed=0, notaps=False, dev=None, zero_s=False, tag=""):
    """flags: words of "s w dl dd f2".  r: radius of the skewed kernel (default: the bucket); n: length of the array it is
    centred in (default 2 r + 1); notaps: no z kernel at all (bucket 0).  dev = (radius, salt): the device taps, same length."""
    fl = flags.split()
    assert set(fl) <= {"s", "w", "dl", "dd", "f2"} and (loss == "depth" or "dd" not in fl), flags
    r = rb if r is None else r
    kz = None if notaps else centred(skewed(r, salt), n)
    dv = None if dev is None else centred(skewed(dev[0], dev[1]), kz.size)
    name = "%s-d%d-%s" % (loss, D, "dyn" if rb is None else "b%d" % rb)
    name += ("-r%d" % r if r != rb else "") + ("-n%d" % n if n else "") + ("-notaps" if notaps else "") + tag
    return Row(name, loss, D, rb, r, kz, dv, "s" in fl, "w" in fl, "dl" in fl, "dd" in fl, 2 if "f2" in fl else 1, seed, zero_s,
               col(loss, D, rb))


MATRIX = [
    # --- expected depth, D = 32
    row("depth", 32, 0, "", notaps=True),
    row("depth", 32, 1, "s w dl dd"),
    row("depth", 32, 2, "s dd"),
    row("depth", 32, 3, "w dl"),
    row("depth", 32, 4, "s w"),
    row("depth", 32, 6, "s dl dd", r=5),
    row("depth", 32, 8, "dd"),
    row("depth", 32, 10, "s w dl f2"),
    row("depth", 32, 15, "s dd"),
    # --- expected depth, D = 64
    row("depth", 64, 0, "s w dd"),
    row("depth", 64, 1, "dl", seed=3),
    row("depth", 64, 2, "s w dl dd f2"),
    row("depth", 64, 3, "s"),
    row("depth", 64, 4, "w dd"),
    row("depth", 64, 6, "s dl", n=21),
    row("depth", 64, 8, "s w dd", r=7),
    row("depth", 64, 10, "dl dd"),
    row("depth", 64, 15, "s w", r=14, salt=0.4),
    # --- expected depth, D = 128
    row("depth", 128, 0, "dl dd", notaps=True),
    row("depth", 128, 1, "s w", salt=2.4, seed=8),
    row("depth", 128, 2, "s dl", seed=7),
    row("depth", 128, 3, "s w dd", n=21),
    row("depth", 128, 4, "s dl dd f2"),
    row("depth", 128, 6, "w"),
    row("depth", 128, 8, "s dd", n=21),
    row("depth", 128, 10, "s w dl dd", r=9),
    row("depth", 128, 15, "s dl", salt=0.4),
    # --- ray-consistency mask, D = 32
    row("drcmask", 32, 0, "s w dl"),
    row("drcmask", 32, 1, "s", salt=3.4),
    row("drcmask", 32, 2, "w dl", seed=2),
    row("drcmask", 32, 3, "s dl", n=21, seed=42),
    row("drcmask", 32, 4, "s w f2", seed=7),
    row("drcmask", 32, 6, "dl", seed=1),
    row("drcmask", 32, 8, "s w dl", r=7, salt=4.9, seed=6),
    row("drcmask", 32, 10, "s", seed=7),
    row("drcmask", 32, 15, "s w", r=14, seed=2),
    # --- ray-consistency mask, D = 64
    row("drcmask", 64, 0, "", notaps=True),
    row("drcmask", 64, 1, "s w dl f2", salt=2.9, seed=2),
    row("drcmask", 64, 2, "s dl", salt=2.9, seed=12),
    row("drcmask", 64, 3, "w", salt=0.4, seed=2),
    row("drcmask", 64, 4, "s dl", salt=2.4, seed=22),
    row("drcmask", 64, 6, "s w", r=5, salt=2.4, seed=1),
    row("drcmask", 64, 8, "", n=21, seed=2),
    row("drcmask", 64, 10, "s w dl", r=9, seed=11),
    row("drcmask", 64, 15, "dl"),
    # --- ray-consistency mask, D = 128
    row("drcmask", 128, 0, "s"),
    row("drcmask", 128, 1, "w dl", salt=2.9, seed=6),
    row("drcmask", 128, 2, "s w", salt=2.9, seed=15),
    row("drcmask", 128, 3, "dl", salt=0.4, seed=16),
    row("drcmask", 128, 4, "dl", salt=3.4, seed=6),
    row("drcmask", 128, 6, "s w dl", n=21, salt=2.4, seed=15),
    row("drcmask", 128, 8, "w", salt=0.4),
    row("drcmask", 128, 10, "dl f2", seed=14),
    row("drcmask", 128, 15, "w dl"),
]

# Asymmetric kernels on the generic kernels: a depth without compiled columns, a z kernel beyond the largest window.
GENERIC = [
    row("depth", 24, None, "s w dl dd f2", r=2),
    row("depth", 32, None, "s dl", r=16),
    row("depth", 40, None, "s dd", r=6),
    row("drcmask", 24, None, "s w dl f2", r=2, salt=2.9, seed=7),
    row("drcmask", 32, None, "s dl", r=16, seed=9),
    row("drcmask", 40, None, "s w", r=6, salt=0.4),
]

# The z taps from device memory.  The host array selects the bucket; the device holds another kernel of the same length and
# of a radius within the bucket (the window's radius or a smaller one); the 21-tap rows have n > 2 RB + 1: resolve_taps' c +- o.
DEVICE = [
    row("depth", 32, 3, "s dl", dev=(3, 0.4), tag="-device"),
    row("depth", 64, 8, "s w dd", dev=(6, 0.4), seed=1, tag="-device"),
    row("depth", 128, 15, "s", dev=(14, 0.4), seed=1, tag="-device"),
    row("depth", 24, None, "s w dl", r=2, dev=(2, 0.4), seed=18, tag="-device"),
    row("depth", 32, 6, "s dd", n=21, dev=(5, 0.4), seed=37, tag="-device"),
    row("drcmask", 32, 3, "w dl", dev=(3, 5.4), seed=56, tag="-device"),
    row("drcmask", 64, 8, "s w", dev=(5, 2.9), seed=14, tag="-device"),
    row("drcmask", 128, 15, "w dl", dev=(13, 0.4), seed=34, tag="-device"),
    row("drcmask", 24, None, "s w dl", r=2, dev=(2, 4.4), seed=14, tag="-device"),
    row("drcmask", 32, 6, "dl", n=21, dev=(5, 0.4), seed=35, tag="-device"),
]

# A cloud with s = 0: no gradient reaches its grid, ds is 0 without a division by s.
ZERO_S = [
    row("depth", 32, 2, "s dl dd", zero_s=True, tag="-zero-s"),
    row("depth", 24, None, "s dd", r=2, zero_s=True, tag="-zero-s"),
    row("drcmask", 32, 2, "s dl", salt=3.4, seed=19, zero_s=True, tag="-zero-s"),
    row("drcmask", 24, None, "s", r=2, salt=2.4, seed=29, zero_s=True, tag="-zero-s"),
]

ROWS = MATRIX + GENERIC + DEVICE + ZERO_S


def applied(r):
    """The taps the device applies: the device values where the row has them."""
    return r.kz if r.dev is None else r.dev


def inputs(r):
    """Seeded fp32 host inputs of a row, generated the way tests/test_drc_loss_gpu.py::mask_inputs does: (grid, s, gt, w, dloss,
    ddepth); gt: depth maps with background pixels, or masks like pooled ones (0, 1 and fractions)."""
    g = torch.Generator().manual_seed(zlib.crc32(r.name.encode()) % 1000000 + r.seed)
    D, f = r.D, r.f
    grid = 0.02 + 1.08 * torch.rand(B, D, G, G, generator=g)
    dens = min(0.45, 4.0 / D)
    grid = grid * (torch.rand(B, D, G, G, generator=g) < dens) * (torch.rand(B, 1, G, G, generator=g) < 0.8)
    s = None
    if r.s:   # the D pass scales an isolated voxel by at most the largest tap: some s v stay beyond 1 at every radius
        s = (0.7 + 1.5 * torch.rand(B, generator=g)) / (1.0 if applied(r) is None else float(applied(r).max()))
        if r.zero_s:
            s[0] = 0.0
    if r.loss == "depth":
        gt = 1.5 + 1.5 * torch.rand(B, f * G, f * G, generator=g)
        gt[torch.rand(B, f * G, f * G, generator=g) < 0.3] = MAX_DATASET_DEPTH
    else:
        gt = (torch.rand(B, f * G, f * G, generator=g) < 0.5).float()
        part = torch.rand(B, f * G, f * G, generator=g) < 0.3
        gt = torch.where(part, torch.rand(B, f * G, f * G, generator=g), gt)
    w = None
    if r.w:
        w = 0.5 + torch.rand(B, generator=g)
        w[0] = 0.0
    dloss = torch.tensor(0.5 + float(torch.rand(1, generator=g))) if r.dloss else None
    ddepth = torch.randn(B, G, G, generator=g) if r.ddepth else None
    return grid.float(), None if s is None else s.float(), gt.float(), w, dloss, ddepth


def oracle(r, taps):
    """dict(loss, depth | None, dgrid, ds | None) of the fp64 oracle on the row's inputs with the z kernel `taps`."""
    grid, s, gt, w, dloss, ddepth = inputs(r)
    gd = grid.double().requires_grad_(True)
    sd = s.double().requires_grad_(True) if s is not None else None
    depth = None
    if r.loss == "depth":
        depth, loss = DO.depth_loss(gd, sd, taps, gt, r.f, w, EPS, CAMERA, MAX_DEPTH, MAX_DATASET_DEPTH)
    else:
        loss = DR.mask_loss(gd, sd, taps, gt, r.f, w, EPS)
    total = loss * (dloss.double() if dloss is not None else 1.0)
    if ddepth is not None:
        total = total + (depth * ddepth.double()).sum()
    total.backward()
    return dict(loss=loss.detach(), depth=None if depth is None else depth.detach(), dgrid=gd.grad,
                ds=None if sd is None else sd.grad)


_REF = {}


def reference(r):
    """The oracle with the taps the device applies, its input conditions asserted; computed once and shared, never changed."""
    if r.name not in _REF:
        grid, s, _, _, _, _ = inputs(r)
        margin = DO.clamp_margin(grid, s, applied(r), EPS)
        assert margin > MARGIN, "%s: a pre-clamp value lies %.2e from a clamp threshold (another seed)" % (r.name, margin)
        if r.s:
            assert float(DO.pre_clamp(grid, s, applied(r)).max()) > 1.0, r.name + ": no s v beyond 1"
        ref = oracle(r, applied(r))
        assert float(ref["dgrid"].abs().max()) > 1e-3, r.name + ": next to no gradient"
        if r.s:
            assert float(ref["ds"].abs().max()) > 0.0, r.name + ": ds is zero"
        if r.loss == "depth":
            assert float(ref["depth"].min()) < 0.9 * MAX_DEPTH, r.name + ": every ray sees the background"
        if r.zero_s:
            assert float(ref["dgrid"][0].abs().max()) == 0.0 and float(ref["ds"][0]) == 0.0 and float(ref["dgrid"][1].abs().max()) > 1e-3
        _REF[r.name] = ref
    return _REF[r.name]


def bound(ref):
    return TOL * max(1.0, float(ref.abs().max()))


def separated(r, other_taps, what):
    """The oracle with `other_taps` lies >= SEPARATION parity bounds from the row's reference, in the loss and in dgrid_wh."""
    ref, other = reference(r), oracle(r, other_taps)
    dl = float((ref["loss"] - other["loss"]).abs())
    dg = float((ref["dgrid"] - other["dgrid"]).abs().max())
    assert dl >= SEPARATION * bound(ref["loss"]), "%s: %s moves the loss by %.2e, %.0f bounds" % (r.name, what, dl, dl / bound(ref["loss"]))
    assert dg >= SEPARATION * bound(ref["dgrid"]), "%s: %s moves dgrid_wh by %.2e, %.0f bounds" % (r.name, what, dg, dg / bound(ref["dgrid"]))


# ------------------------------------------------------------------------------------------------------ CPU: the gate
def test_matrix_names_every_column_instantiation_in_the_build():
    """The kernel symbols of dpc_depth.o, dpc_drc_loss.o and dpc_rgb.o == (what the rows claim) + ELSEWHERE, exactly."""
    built = built_instantiations(COLUMN_OBJECTS)
    matrix = set().union(*(r.ids for r in MATRIX))
    assert len(matrix) == 2 * 2 * len(DEPTHS) * len(BUCKETS)
    claimed = set().union(*(r.ids for r in ROWS))
    assert claimed - matrix <= set(ELSEWHERE), "rows outside the matrix launch the generic kernels only"
    missing = sorted(built - claimed - set(ELSEWHERE))
    stale = sorted((claimed | set(ELSEWHERE)) - built)
    assert not missing, "instantiations no row launches (add a row, or an ELSEWHERE entry with the file that pins it): %s" % missing
    assert not stale, "rows / ELSEWHERE entries naming instantiations the build does not contain: %s" % stale
    here = os.path.dirname(os.path.abspath(__file__))
    for kid, (name, needle) in ELSEWHERE.items():
        with open(os.path.join(here, name)) as fh:
            assert needle in fh.read(), "%s: %s does not mention %s" % (kid, name, needle)


def test_matrix_has_one_row_per_cell_and_spreads_the_options():
    """CPU check of the table itself: 54 rows, every (loss, D, bucket) once; each option on and off with several buckets at
    each depth; the radii and array lengths the docstring promises."""
    cells = [(r.loss, r.D, r.rb) for r in MATRIX]
    assert sorted(cells) == sorted((l, D, b) for l in ("depth", "drcmask") for D in DEPTHS for b in BUCKETS)
    assert len({r.name for r in ROWS}) == len(ROWS)
    for loss in ("depth", "drcmask"):
        for D in DEPTHS:
            rows = [r for r in MATRIX if (r.loss, r.D) == (loss, D)]
            for opt in ("s", "w", "dloss") + (("ddepth",) if loss == "depth" else ()):
                on = sum(1 for r in rows if getattr(r, opt))
                assert 3 <= on <= len(rows) - 2, (loss, D, opt, on)
    assert sum(1 for r in MATRIX if r.f == 2) >= 4
    for b in (6, 8, 10, 15):    # the window's ends zero
        assert any(r.rb == b and r.r == b - 1 for r in MATRIX), b
    padded = [r for r in MATRIX if r.kz is not None and r.kz.size == 21 and r.r < 10]
    assert len(padded) >= 3 and {r.r for r in padded} == {3, 6, 8}
    for r in padded:
        c = (r.kz.size - 1) // 2
        assert not r.kz[:c - r.r].any() and not r.kz[c + r.r + 1:].any() and r.kz[c - r.r] > 0 and r.kz[c + r.r] > 0


def test_rows_ask_for_the_buckets_they_claim():
    """Every row's HOST kernel needs the bucket its ids carry (dpc_taps_bucket), is asymmetric and keeps every tap of its
    core; the device taps have the host array's length and stay within the window."""
    import dpc.render as R

    for r in ROWS:
        if r.kz is None:
            assert r.rb == 0 and r.dev is None, r.name
            continue
        bucket = R.taps_bucket(r.kz)
        if r.rb is None:
            assert bucket == -1 or r.D not in DEPTHS, (r.name, bucket)
        else:
            assert bucket == r.rb and r.D in DEPTHS, (r.name, bucket)
        core = r.kz[r.kz != 0]
        assert core.size == 2 * r.r + 1 and core.min() > 1e-4 * core.sum(), r.name
        assert r.r == 0 or not np.array_equal(r.kz, r.kz[::-1]), r.name + ": the kernel is symmetric"
        if r.dev is not None:
            assert r.dev.size == r.kz.size and not np.array_equal(r.dev, r.kz) and not np.array_equal(r.dev, r.dev[::-1]), r.name
            assert r.rb is None or 0 <= R.taps_bucket(r.dev) <= r.rb, r.name


@pytest.mark.parametrize("r", ROWS, ids=[r.name for r in ROWS])
def test_rows_meet_their_input_conditions(r):
    """The conditions on the seeded inputs, on the oracle alone (reference() asserts them)."""
    reference(r)


@pytest.mark.parametrize("r", [r for r in ROWS if r.r > 0], ids=[r.name for r in ROWS if r.r > 0])
def test_rows_tell_a_flipped_kernel_apart(r):
    """The oracle with kz[::-1] lies >= 100 parity bounds from the oracle with kz: the skew cannot hide inside the tolerance."""
    separated(r, np.ascontiguousarray(applied(r)[::-1]), "flipping the kernel")


@pytest.mark.parametrize("r", DEVICE, ids=[r.name for r in DEVICE])
def test_device_rows_tell_the_host_taps_apart(r):
    """The oracle with the HOST values lies >= 100 parity bounds from the oracle with the device values."""
    separated(r, r.kz, "taking the host's taps")


# ------------------------------------------------------------------------------------------------------ GPU: the matrix
def run_abi(r):
    """The row through the two C entry points of its loss; returns device tensors (loss, depth | None, dgrid_wh, ds | None),
    the launch lists of the forward and of the backward, and the tickets' largest value after the backward."""
    from dpc.render import _native as N

    grid, s, gt, w, dloss, ddepth = (None if x is None else x.cuda().contiguous() for x in inputs(r))
    D = r.D
    kz = None if r.kz is None else np.ascontiguousarray(r.kz, dtype=np.float32)
    dev_taps = None
    if r.dev is not None:   # a DeviceSchedule's taps_z: DPC_MAX_TAPS values, the kernel's in front
        dev_taps = torch.zeros(N.DPC_MAX_TAPS, dtype=torch.float32)
        dev_taps[:r.dev.size] = torch.from_numpy(r.dev)
        dev_taps = dev_taps.cuda()
    depth_loss = r.loss == "depth"
    P = N.DpcParams(B, 0, D, G, G, 0, 0 if kz is None else kz.size, CAMERA, 1.875, EPS, MAX_DEPTH if depth_loss else 10.0, 1, 0,
                    None, None, None, None, N.ptr(dev_taps))
    ref, L, st = ctypes.byref(P), N.lib(), N.stream_ptr(torch.device("cuda"))
    kzp = None if kz is None else kz.ctypes.data_as(ctypes.c_void_p)
    nan = float("nan")
    depth = torch.full((B, G, G), nan, device="cuda") if depth_loss else None
    tiles = torch.full((B, (G * G + 255) // 256), nan, device="cuda")
    loss = torch.full((1,), nan, device="cuda")
    dgrid = torch.full((B, D, G, G), nan, device="cuda")     # overwritten: no pre-zeroing
    ds = torch.full((B,), nan, device="cuda") if s is not None else None
    # the caller's part of the workspace contract: the tickets (first 4 * B bytes) zeroed once; the rest may hold anything
    nbytes = (L.dpc_depth_workspace_bytes if depth_loss else L.dpc_drc_workspace_bytes)(ref)
    ws = torch.full((max(nbytes, 16),), 0xA5, dtype=torch.uint8, device="cuda")
    ws[:4 * B] = 0

    def fwd():
        if depth_loss:
            N.check(L.dpc_depth_loss_fwd(ref, N.ptr(grid), N.ptr(s), kzp, N.ptr(gt), r.f, MAX_DATASET_DEPTH, N.ptr(w), N.ptr(depth),
                                         N.ptr(tiles), N.ptr(loss), st), "dpc_depth_loss_fwd")
        else:
            N.check(L.dpc_drc_loss_fwd(ref, N.ptr(grid), N.ptr(s), kzp, N.ptr(gt), r.f, N.ptr(w), N.ptr(tiles), N.ptr(loss), st),
                    "dpc_drc_loss_fwd")

    def bwd():
        if depth_loss:
            N.check(L.dpc_depth_loss_bwd(ref, N.ptr(grid), N.ptr(s), kzp, N.ptr(gt), r.f, MAX_DATASET_DEPTH, N.ptr(w), N.ptr(dloss),
                                         N.ptr(ddepth), N.ptr(dgrid), N.ptr(ds), N.ptr(ws), st), "dpc_depth_loss_bwd")
        else:
            N.check(L.dpc_drc_loss_bwd(ref, N.ptr(grid), N.ptr(s), kzp, N.ptr(gt), r.f, N.ptr(w), N.ptr(dloss), N.ptr(dgrid),
                                       N.ptr(ds), N.ptr(ws), st), "dpc_drc_loss_bwd")

    lf, lb = launch_list(fwd), launch_list(bwd)
    return loss, depth, dgrid, ds, lf, lb, int(ws[:4 * B].max())


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=[r.name for r in ROWS])
def test_column_vs_oracle(r):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    ref = reference(r)
    loss, depth, dgrid, ds, lf, lb, tickets = run_abi(r)
    assert lf == [r.ids[0], FIN] and lb == [r.ids[1]], "%s: launched %s and %s, the row expects %s" % (r.name, lf, lb, r.ids)
    tag = "column %s: " % r.name
    close(loss[0], ref["loss"], TOL, tag + "loss")
    if depth is not None:
        close(depth, ref["depth"], TOL, tag + "depth")
    close(dgrid, ref["dgrid"], TOL, tag + "dgrid_wh")
    if r.s:
        close(ds, ref["ds"], TOL, tag + "ds")
    assert tickets == 0, r.name + ": the backward left a ticket behind"
    if r.zero_s:
        assert float(dgrid[0].abs().max()) == 0.0, r.name + ": gradient in the grid of the cloud with s = 0"
        assert float(ds[0]) == 0.0 and bool(torch.isfinite(ds).all()), r.name


# ------------------------------------------------------------------------------------------------------ GPU: a DeviceSchedule
SCHED = dict(B=4, N=500, G=32, rxy=1, rz=3, rz_new=2, f=2)


def sched_kernels():
    """([kx, ky, kz] the projection is built with, the same list with the narrower z kernel the schedule moves to)."""
    kx, kz = torch.from_numpy(skewed(SCHED["rxy"], 0.3)), torch.from_numpy(skewed(SCHED["rz"], 1.9))
    kz_new = torch.from_numpy(centred(skewed(SCHED["rz_new"], 0.4), kz.numel()))
    n, nz = kx.numel(), kz.numel()
    lst = lambda z: [kx.reshape(1, 1, 1, 1, n), kx.reshape(1, 1, 1, n, 1), z.reshape(1, 1, nz, 1, 1)]
    return lst(kz), lst(kz_new)


def sched_cfg(O):
    return O.Cfg(vox_size=SCHED["G"], pc_gauss_kernel_size=2 * SCHED["rxy"] + 1, max_depth=MAX_DEPTH,
                 max_dataset_depth=MAX_DATASET_DEPTH, drc_logsum_clip_val=EPS)


def sched_inputs(O):
    """Points, poses, scales, translations, focal lengths, depth maps and weights of test_depth_loss_gpu.e2e_inputs (points
    constructed in the grid, so that the clamp margins hold), and masks like pooled ones."""
    pc, q, s, t, f, depths, w, _ = e2e_inputs(O, False, SCHED["B"], SCHED["N"], SCHED["G"])
    g = torch.Generator().manual_seed(77)
    shape = (SCHED["B"], SCHED["f"] * SCHED["G"], SCHED["f"] * SCHED["G"])
    masks = (torch.rand(shape, generator=g) < 0.5).float()
    masks = torch.where(torch.rand(shape, generator=g) < 0.3, torch.rand(shape, generator=g), masks)
    return pc, q, s, t, f, depths, w, masks


_SCHED = {}


def sched_reference(O):
    """oracle/dpc_oracle.py with the UPDATED z taps, then the two loss oracles: losses and gradients (points, q, s, t, f)."""
    if not _SCHED:
        cfg, (_, kern) = sched_cfg(O), sched_kernels()
        pc, q, s, t, f, depths, w, masks = sched_inputs(O)
        leaves = [x.clone().requires_grad_(True) for x in (pc, q, s, t, f)]
        ref = O.pointcloud_project_fast(cfg, leaves[0], leaves[1], leaves[3], None, kern, scaling_factor=leaves[2], focal_length=leaves[4])
        vox = O.smoothen_voxels3d(cfg, torch.clamp(ref["voxels_raw"].unsqueeze(1), 0.0, 1.0), kern).squeeze(1)
        x = (vox * leaves[2].double().reshape(-1, 1, 1, 1)).detach().reshape(-1)
        x = x[x != 0]
        margin = min(float((x - v).abs().min()) for v in (EPS, 1.0 - EPS, 1.0))
        assert margin > MARGIN, "a pre-clamp value lies %.2e from a clamp threshold" % margin
        assert x.numel() > 20000 and float(ref["voxels_raw"].detach().sum()) > 0.95 * pc.shape[0] * pc.shape[1]   # the points are in the grid
        depth_loss = DO.loss_of_depth(ref["proj_depth"][..., 0], depths[..., 0], SCHED["f"], w, cfg.max_depth, MAX_DATASET_DEPTH)
        mask_loss = DR.mask_loss_of_probabilities(ref["drc_probs"][..., 0].permute(1, 0, 2, 3), masks, SCHED["f"], w)
        (depth_loss + mask_loss).backward()
        _SCHED.update(depth=depth_loss.detach(), mask=mask_loss.detach(), grads=[x.grad for x in leaves])
    return _SCHED


@pytest.fixture(scope="module")
def O():
    from oracle import dpc_oracle as O

    O.EXACT_POSE_GRADIENT = True   # d(q) against the exact fp64 sum over the points, as tests/test_gpu_parity.py does
    yield O
    O.EXACT_POSE_GRADIENT = False


def test_schedule_case_inputs(O):
    """CPU: the z kernel the schedule moves to is asymmetric, another kernel, and fits the bucket of the one it was built
    with; the clamp margins of the constructed points hold under it (sched_reference asserts them)."""
    import dpc.render as R

    old, new = (k[2].reshape(-1).numpy() for k in sched_kernels())
    assert R.taps_bucket(old) == 3 and 0 <= R.taps_bucket(new) <= 3 and old.size == new.size
    assert not np.array_equal(new, new[::-1]) and float(np.abs(old - new).max()) > 0.05
    ref = sched_reference(O)
    assert float(ref["depth"]) > 0 and float(ref["mask"]) > 0


@pytest.mark.gpu
def test_losses_follow_a_device_schedule(O):
    """pointcloud_project_fast under a DeviceSchedule, the schedule moved to a narrower asymmetric z kernel, then
    proj_depth_loss + drc_loss with backward: the loss columns read the z taps from device memory (the grid they start from has
    been through the W and H passes only, so it is the same under both z kernels)."""
    import dpc.render as R
    from dpc.render import _native

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    ref = sched_reference(O)
    cfg, (kern, kern_new) = sched_cfg(O), sched_kernels()
    pc, q, s, t, f, depths, w, masks = sched_inputs(O)
    d = torch.device("cuda")
    leaves = [x.to(d, torch.float32).requires_grad_(True) for x in (pc, q, s, t, f)]
    sched = R.DeviceSchedule(d, kern[0].reshape(-1).numpy(), kern[2].reshape(-1).numpy())
    out = R.pointcloud_project_fast(cfg, leaves[0], leaves[1], leaves[3], None, kern, scaling_factor=leaves[2],
                                    focal_length=leaves[4], schedule=sched)
    sched.update(kern_new[0].reshape(-1).numpy(), kern_new[2].reshape(-1).numpy())
    got = {}

    def losses():
        got["depth"] = R.proj_depth_loss(cfg, out, depths.to(d), w.to(d))
        got["mask"] = R.drc_loss(cfg, out, masks.to(d), w.to(d))
        (got["depth"] + got["mask"]).backward()

    ids = _native.launched_instantiations(losses, d)
    want = set(col("depth", SCHED["G"], 3)) | set(col("drcmask", SCHED["G"], 3)) | {FIN}
    assert want <= ids, "launched %s, expected %s among them" % (sorted(ids), sorted(want))
    close(got["depth"], ref["depth"], TOL, "column schedule: depth loss")
    close(got["mask"], ref["mask"], TOL, "column schedule: mask loss")
    for name, x, r in zip(("points", "quaternions", "s", "t", "f"), leaves, ref["grads"]):
        assert x.grad is not None and float(r.abs().max()) > 0, name
        close(x.grad, r, TOL, "column schedule: d(%s)" % name)


@pytest.mark.gpu
def test_zz_column_matrix_error_report():
    """Not a check: rewrites the suite's margin report (tests/test_gpu_parity.py::test_zz_error_report) so that it holds this
    module's comparisons -- they go into the same ERRORS list."""
    import test_gpu_parity

    assert any(what.startswith("column ") for what, _, _ in ERRORS)
    test_gpu_parity.test_zz_error_report()
