"""Every kernel instantiation of the fused path against the oracle, once.

The fused path is a table of template instantiations picked at run time by the launchers (csrc/dpc_slab_fwd.hip,
dpc_slab_xl.hip, dpc_slab_bwd.hip, dpc_column.hip) from the grid width, the radius buckets of the x/y and z kernels
(plan_taps: 0, 1, 2, 3, 4, 6, 8, 10, 15), the depth, the number of clouds with backward work and the call shape.  Each is
separately compiled code with its own register window, LDS layout and pad width, so each answers to the oracle here:

  - CASES is a declarative table; a row names the call and THE SET OF INSTANTIATIONS IT MUST LAUNCH.  The GPU case checks
    that set against the library's launch record (dpc_profile_get_id), so a launcher whose choice drifts fails the case
    instead of silently testing something else, and compares the results with oracle/dpc_oracle.py under the parity rule
    of tests/test_gpu_parity.py: max|dev - ref| <= 1e-5 * max(1, max|ref|).
  - The kernels are positive, normalised and ASYMMETRIC (a backward that correlates where it should convolve fails), with
    outer taps far above plan_taps' 1e-8 drop threshold, so the effective radius is the one the row means: most rows fill
    the register window (radius = bucket), some leave its ends zero (radius = bucket - 1).  A few rows use the symmetric
    Gaussian of smoothing_kernel, the only case in which k_splat_xl takes its Horner W pass.
  - test_matrix_names_every_instantiation_in_the_build (CPU) reads the kernel symbols of the four fused-path device objects
    and asserts they are exactly the rows' instantiations plus UNREACHABLE: deleting a row, or adding an instantiation to a
    launcher, fails the CPU suite.

Grids: the Python API has square H = W planes (vox_size) and a depth of its own (vox_size_z); a grid's "box" shape here is
D != H.  Rows with many clouds (the thick 64-wide backward slabs need B * ceil(D / 8) >= 256) check the oracle on the
samples listed in `sub` -- every cloud's results depend on its own inputs only."""
from collections import namedtuple

import numpy as np
import pytest
import torch

from test_abi_and_host import device_object_output
from test_gpu_parity import ERRORS, TOL, close

BUCKETS = (0, 1, 2, 3, 4, 6, 8, 10, 15)
FUSED_OBJECTS = ("dpc_slab_fwd.o", "dpc_slab_xl.o", "dpc_slab_bwd.o", "dpc_column.o")


def sp(G, ZS, RB):
    return "k_splat_hw<%d, %d, %d>" % (G, ZS, RB)


def xl(RB):
    return "k_splat_xl<4, %d>" % RB


def ga(G, ZS, RB):
    return "k_gather_hw<%d, %d, %d>" % (G, ZS, RB)


def zcol(D, RB):   # the plain forward + backward column pair
    return ("k_zcol_fwd<%d, %d>" % (D, RB), "k_zcol_bwd<%d, %d>" % (D, RB))


def zfb(D, RB):    # the forward with the column backward fused in (one pose candidate per sample, K = 1)
    return ("k_zcol_fwdbwd<%d, %d, 1>" % (D, RB),)


ZDYN = ("k_zcol_fwd_dyn", "k_zcol_bwd_dyn")
LOC = "k_locate<0>"
FIN = "k_loss_finalize"
FIX = "k_fixed_to_dpc"

# Instantiations that the build contains and no call of this library can launch, with the launcher line that rules them out.
_XL = ("dpc_slab_fwd.hip launch_splat: 64 x 64 planes at buckets 1, 2, 3, 4, 6 go to k_splat_xl (xl_applies) whenever the "
       "W/H passes run (Tbuf != nullptr) and no raw grid is asked for; a raw grid takes the generic kernel "
       "(launch_splat_rb: raw_with_passes), and Tbuf is nullptr only for dpc_splat_fwd, at bucket 0.  Built for -DDPC_NO_XL.")
UNREACHABLE = {sp(64, 4, rb): _XL for rb in (1, 2, 3, 4, 6)}

# path: "plain" = pointcloud_project_fast + backward of sum(proj * w); "fwd" = forward only; "loss" = pointcloud_project_loss
# (K candidates) + backward; "step" = project_loss_step(...).run(); "locate" = pointcloud2voxels3d_fast of transformed points
# (fp32 or fp64) + backward.  rxy / rz: radius of the skewed kernels, or ("gauss", sigma): smoothing_kernel(cfg, sigma) for
# both.  R: clouds per shared point set; keep: point_index with this keep fraction; sub: samples the oracle checks (None = all);
# clamp_flip: the input has a voxel at the DRC clamp's threshold that the device decides the other way (judged, see below).
Case = namedtuple("Case", "name G D B N path rxy rz ids K R keep t f sched sub seed clamp_flip")


def case(name, G, D, B, N, path, rxy, rz, ids, K=1, R=1, keep=None, t=False, f=False, sched=False, sub=None, seed=0,
         clamp_flip=False):
    return Case(name, G, D, B, N, path, rxy, rz, frozenset(ids), K, R, keep, t, f, sched, sub, seed, clamp_flip)


CASES = [
    # --- 32-wide LDS-window kernels k_splat_hw / k_gather_hw<32, 4, RB>; columns at D = 128
    case("w32-b0", 32, 128, 3, 2500, "plain", 0, 0, [LOC, sp(32, 4, 0), *zcol(128, 0), ga(32, 4, 0)]),
    case("w32-b1", 32, 128, 3, 2500, "loss", 1, 1, [LOC, sp(32, 4, 1), *zfb(128, 1), ga(32, 4, 1)], t=True),
    case("w32-b2", 32, 128, 3, 2500, "plain", 2, 2, [LOC, sp(32, 4, 2), *zcol(128, 2), ga(32, 4, 2)], f=True),
    case("w32-b3", 32, 128, 3, 2500, "loss", 3, 3, [LOC, sp(32, 4, 3), *zfb(128, 3), ga(32, 4, 3)]),
    case("w32-b4", 32, 128, 5, 2500, "plain", 4, 4, [LOC, sp(32, 4, 4), *zcol(128, 4), ga(32, 4, 4)], t=True, f=True),
    case("w32-b6", 32, 128, 3, 2500, "loss", 5, 6, [LOC, sp(32, 4, 6), *zfb(128, 6), ga(32, 4, 6)]),
    case("w32-b8", 32, 128, 3, 2500, "plain", 8, 7, [LOC, sp(32, 4, 8), *zcol(128, 8), ga(32, 4, 8)]),
    case("w32-b10", 32, 128, 3, 2500, "loss", 10, 10, [LOC, sp(32, 4, 10), *zfb(128, 10), ga(32, 4, 10)], f=True),
    # --- 128-wide one-layer kernels <128, 1, RB>; columns at D = 32
    case("w128-b0", 128, 32, 2, 12000, "loss", 0, 0, [LOC, sp(128, 1, 0), *zfb(32, 0), ga(128, 1, 0)]),
    case("w128-b1", 128, 32, 2, 12000, "plain", 1, 1, [LOC, sp(128, 1, 1), *zcol(32, 1), ga(128, 1, 1)], t=True),
    case("w128-b2", 128, 32, 2, 12000, "loss", 2, 2, [LOC, sp(128, 1, 2), *zfb(32, 2), ga(128, 1, 2)]),
    case("w128-b3", 128, 32, 2, 12000, "plain", 3, 3, [LOC, sp(128, 1, 3), *zcol(32, 3), ga(128, 1, 3)], f=True),
    case("w128-b4", 128, 32, 2, 12000, "loss", 4, 4, [LOC, sp(128, 1, 4), *zfb(32, 4), ga(128, 1, 4)]),
    case("w128-b6", 128, 32, 2, 12000, "plain", 6, 6, [LOC, sp(128, 1, 6), *zcol(32, 6), ga(128, 1, 6)]),
    case("w128-b8", 128, 32, 2, 12000, "loss", 7, 8, [LOC, sp(128, 1, 8), *zfb(32, 8), ga(128, 1, 8)], t=True, f=True),
    case("w128-b10", 128, 32, 2, 12000, "plain", 10, 9, [LOC, sp(128, 1, 10), *zcol(32, 10), ga(128, 1, 10)]),
    # --- 64-wide, THICK backward slabs <64, 8, RB>: B * ceil(D / 8) >= 256 clouds' worth of work
    case("w64-thick-b0", 64, 64, 33, 5000, "plain", 0, 0, [LOC, sp(64, 4, 0), *zcol(64, 0), ga(64, 8, 0)], sub=[0, 32]),
    case("w64-thick-b1", 64, 64, 32, 5000, "loss", 1, 1, [LOC, xl(1), *zfb(64, 1), ga(64, 8, 1)], sub=[3, 31], t=True),
    case("w64-thick-b2", 64, 32, 64, 4000, "plain", 2, 2, [LOC, xl(2), *zcol(32, 2), ga(64, 8, 2)], sub=[0, 63]),
    case("w64-thick-b3", 64, 64, 32, 5000, "step", 3, 3, [LOC, xl(3), *zfb(64, 3), ga(64, 8, 3)], sub=[5, 30], t=True, f=True),
    case("w64-thick-b4", 64, 128, 16, 5000, "loss", 4, 4, [LOC, xl(4), *zfb(128, 4), ga(64, 8, 4)], sub=[1, 15]),
    case("w64-thick-b6", 64, 64, 33, 5000, "plain", 6, 5, [LOC, xl(6), *zcol(64, 6), ga(64, 8, 6)], sub=[2, 32]),
    case("w64-thick-b8", 64, 32, 65, 4000, "plain", 8, 8, [LOC, sp(64, 4, 8), *zcol(32, 8), ga(64, 8, 8)], sub=[0, 64]),
    case("w64-thick-b10", 64, 128, 16, 5000, "loss", 9, 15, [LOC, sp(64, 4, 10), *zfb(128, 15), ga(64, 8, 10)], sub=[0, 9]),
    # --- 64-wide, THIN backward slabs <64, 4, RB <= 4> and WIDE ones <64, 3, {6, 8, 10}>: few clouds
    case("w64-thin-b0", 64, 64, 3, 4000, "loss", 0, 0, [LOC, sp(64, 4, 0), *zfb(64, 0), ga(64, 4, 0)]),
    case("w64-thin-b1", 64, 64, 3, 4000, "plain", 1, 1, [LOC, xl(1), *zcol(64, 1), ga(64, 4, 1)], f=True),
    case("w64-thin-b2", 64, 128, 3, 4000, "loss", 2, 2, [LOC, xl(2), *zfb(128, 2), ga(64, 4, 2)]),
    case("w64-thin-b3", 64, 64, 3, 4000, "loss", 3, 2, [LOC, xl(3), *zfb(64, 2), ga(64, 4, 3)], t=True),
    case("w64-thin-b4", 64, 128, 3, 4000, "loss", 4, 0, [LOC, xl(4), *zfb(128, 0), ga(64, 4, 4)]),
    case("w64-wide-b6", 64, 64, 3, 4000, "plain", 6, 4, [LOC, xl(6), *zcol(64, 4), ga(64, 3, 6)]),
    case("w64-wide-b8", 64, 128, 3, 4000, "loss", 8, 8, [LOC, sp(64, 4, 8), *zfb(128, 8), ga(64, 3, 8)]),
    case("w64-wide-b10", 64, 64, 3, 4000, "plain", 10, 10, [LOC, sp(64, 4, 10), *zcol(64, 10), ga(64, 3, 10)], t=True),
    # --- k_splat_xl's Horner W pass (symmetric Gaussians only) at every xl bucket
    case("w64-gauss-b1", 64, 128, 3, 4000, "plain", ("gauss", 0.25), ("gauss", 0.25), [LOC, xl(1), *zcol(128, 3), ga(64, 4, 1)]),
    case("w64-gauss-b2", 64, 64, 3, 4000, "plain", ("gauss", 0.4), ("gauss", 0.4), [LOC, xl(2), *zcol(64, 2), ga(64, 4, 2)]),
    case("w64-gauss-b3", 64, 128, 3, 4000, "plain", ("gauss", 0.6), ("gauss", 0.6), [LOC, xl(3), *zcol(128, 8), ga(64, 4, 3)]),
    case("w64-gauss-b4", 64, 32, 3, 4000, "plain", ("gauss", 0.75), ("gauss", 0.75), [LOC, xl(4), *zcol(32, 2), ga(64, 4, 4)]),
    case("w64-gauss-b6", 64, 128, 3, 4000, "plain", ("gauss", 1.0), ("gauss", 1.0), [LOC, xl(6), *zcol(128, 15), ga(64, 3, 6)],
         clamp_flip=True),
    case("w32-gauss-b3", 32, 32, 3, 2500, "loss", ("gauss", 0.6), ("gauss", 0.6), [LOC, sp(32, 4, 3), *zfb(32, 3), ga(32, 4, 3)]),
    # --- k_splat_xl reading its taps from device memory (a DeviceSchedule: the step plan's taps), asymmetric
    case("w64-xl-device-taps", 64, 64, 3, 4000, "step", 3, 6, [LOC, xl(3), *zfb(64, 6), ga(64, 4, 3)], sched=True),
    # --- generic kernels <0, 0, RB> (widths without kernels of their own; bucket 15 on every width), 64-bit accumulators
    case("gen-b0", 24, 128, 3, 1500, "plain", 0, 10, [LOC, sp(0, 0, 0), *zcol(128, 10), ga(0, 0, 0)]),
    case("gen-b1-box", 48, 40, 3, 3000, "plain", 1, 3, [LOC, sp(0, 0, 1), *ZDYN, ga(0, 0, 1)], t=True, f=True),
    case("gen-b2", 40, 32, 5, 2500, "plain", 2, 14, [LOC, sp(0, 0, 2), *zcol(32, 15), ga(0, 0, 2)]),
    case("gen-b3", 24, 128, 3, 1500, "plain", 3, 15, [LOC, sp(0, 0, 3), *zcol(128, 15), ga(0, 0, 3)]),
    case("gen-b4", 96, 32, 2, 8000, "plain", 4, 0, [LOC, sp(0, 0, 4), *zcol(32, 0), ga(0, 0, 4)]),
    case("gen-b6", 24, 64, 3, 1500, "loss", 6, 15, [LOC, sp(0, 0, 6), *zfb(64, 15), ga(0, 0, 6)], f=True),
    case("gen-b8", 40, 64, 3, 2500, "plain", 8, 15, [LOC, sp(0, 0, 8), *zcol(64, 15), ga(0, 0, 8)]),
    case("gen-b10-zdyn", 24, 64, 3, 1500, "plain", 10, 18, [LOC, sp(0, 0, 10), *ZDYN, ga(0, 0, 10)]),
    case("gen-b15-square", 32, 32, 3, 2500, "loss", 15, 15, [LOC, sp(0, 0, 15), *zfb(32, 15), ga(0, 0, 15)]),
    case("gen-b15-w64", 64, 32, 2, 4000, "plain", 14, 4, [LOC, sp(0, 0, 15), *zcol(32, 4), ga(0, 0, 15)]),
    # generic forward with fp32 LDS accumulators: planes 142..199 wide, no backward there
    case("gen-fp32-acc-fwd", 150, 32, 2, 12000, "fwd", 3, 6, [LOC, sp(0, 0, 3), "k_zcol_fwd<32, 6>"]),
    # --- the remaining column cells
    case("w32-zcol128-b1", 32, 128, 3, 2500, "plain", 2, 1, [LOC, sp(32, 4, 2), *zcol(128, 1), ga(32, 4, 2)], seed=1),
    case("w32-zcol128-b6", 32, 128, 3, 2500, "plain", 4, 6, [LOC, sp(32, 4, 4), *zcol(128, 6), ga(32, 4, 4)], seed=1),
    case("w32-zfb64-b8", 32, 64, 3, 2500, "loss", 8, 8, [LOC, sp(32, 4, 8), *zfb(64, 8), ga(32, 4, 8)], t=True, f=True),
    case("w32-zfb64-b10", 32, 64, 5, 2500, "step", 10, 10, [LOC, sp(32, 4, 10), *zfb(64, 10), ga(32, 4, 10)]),
    case("w32-zfb32-b1", 32, 32, 3, 2500, "step", 4, 1, [LOC, sp(32, 4, 4), *zfb(32, 1), ga(32, 4, 4)], f=True),
    case("gen-zfb32-b3", 40, 32, 3, 2500, "loss", 0, 3, [LOC, sp(0, 0, 0), *zfb(32, 3), ga(0, 0, 0)]),
    case("w64-zfb32-b6", 64, 32, 3, 4000, "loss", 2, 5, [LOC, xl(2), *zfb(32, 6), ga(64, 4, 2)]),
    case("w32-zfb32-b10", 32, 32, 3, 2500, "loss", 6, 10, [LOC, sp(32, 4, 6), *zfb(32, 10), ga(32, 4, 6)]),
    case("w64-zfb64-b4-shared", 64, 64, 6, 4000, "loss", 4, 4, [LOC, xl(4), *zfb(64, 4), ga(64, 4, 4), FIX], R=3),
    # --- K > 1 pose candidates: the finalize launch, the plain column backward and winners-only gathers
    case("w32-K4-shared-single-writer", 32, 64, 8, 2500, "loss", 3, 3,
         [LOC, sp(32, 4, 3), *zcol(64, 3), FIN, ga(32, 4, 3)], K=4, R=4),
    case("gen-K2-point-index", 48, 32, 8, 2000, "loss", 6, 6,
         [LOC, sp(0, 0, 6), *zcol(32, 6), FIN, ga(0, 0, 6), FIX], K=2, R=4, keep=0.6),
    # the one-call step with K > 1: the min-of-K selection made inside k_zcol_bwd (no finalize launch)
    case("w64-step-K4-shared", 64, 64, 8, 4000, "step", 8, 8, [LOC, sp(64, 4, 8), *zcol(64, 8), ga(64, 3, 8)], K=4, R=4),
    # per-cloud gathers into shared point sets / point_index subsets (64-bit fixed-point point gradients)
    case("w32-plain-point-index", 32, 32, 6, 2500, "plain", 1, 2, [LOC, sp(32, 4, 1), *zcol(32, 2), ga(32, 4, 1), FIX],
         R=2, keep=0.7),
    # --- k_locate from already-transformed points (pointcloud2voxels3d_fast): fp32 and fp64, and the bucket-0 splats
    case("locate-f32-w32", 32, 32, 3, 3000, "locate", None, None, ["k_locate<1>", sp(32, 4, 0)], keep="f32"),
    case("locate-f64-w128", 128, 16, 2, 12000, "locate", None, None, ["k_locate<2>", sp(128, 1, 0)], keep="f64"),
    case("locate-f32-w64", 64, 40, 3, 4000, "locate", None, None, ["k_locate<1>", sp(64, 4, 0)], keep="f32"),
    case("locate-f64-gen", 40, 24, 3, 2500, "locate", None, None, ["k_locate<2>", sp(0, 0, 0)], keep="f64"),
]


def skewed(r, salt):
    """Positive, normalised, asymmetric 1-D kernel of radius r whose every tap weighs > 1e-4 of the total (far above plan_taps'
    1e-8 drop threshold): the effective radius is r."""
    if r == 0:
        return np.ones(1, np.float32)
    i = np.arange(-r, r + 1, dtype=np.float64)
    k = np.exp(-((i + 0.35 * r) ** 2) / (2 * (0.8 * r + 0.5) ** 2)) * (1.0 + 0.3 * np.sin(1.7 * i + salt))
    return (k / k.sum()).astype(np.float32)


def kernels(c, O):
    """(cfg, kernel list [kx, ky, kz]) of a row: skewed kernels, or smoothing_kernel's Gaussian."""
    if c.path == "locate":
        return O.Cfg(vox_size=c.G, vox_size_z=c.D), None
    if isinstance(c.rxy, tuple):
        cfg = O.Cfg(vox_size=c.G, vox_size_z=c.D, pc_gauss_kernel_size=21)
        return cfg, [k.clone() for k in O.smoothing_kernel(cfg, c.rxy[1])]
    kx, kz = torch.from_numpy(skewed(c.rxy, 0.3 + c.seed)), torch.from_numpy(skewed(c.rz, 1.9 + c.seed))
    cfg = O.Cfg(vox_size=c.G, vox_size_z=c.D, pc_gauss_kernel_size=kx.numel())
    n, nz = kx.numel(), kz.numel()
    return cfg, [kx.reshape(1, 1, 1, 1, n), kx.reshape(1, 1, 1, n, 1), kz.reshape(1, 1, nz, 1, 1)]


def _planned(k):
    """k with the outer taps zeroed that plan_taps drops (csrc/dpc_kernels.h: pairs whose running |weight| stays within 1e-8
    of the total), i.e. the taps the fused kernels run."""
    flat = k.reshape(-1).double()
    c = (flat.numel() - 1) // 2
    total, dropped, r = float(flat.abs().sum()), 0.0, c
    while r > 0:
        d = abs(float(flat[c - r])) + abs(float(flat[c + r]))
        if dropped + d > 1e-8 * total:
            break
        dropped += d
        r -= 1
    out = flat.clone()
    out[:c - r] = 0.0
    out[c + r + 1:] = 0.0
    return out.reshape(k.shape)


def _seed(c):
    return 7000 + 97 * CASES.index(c) + c.seed


def _family(i):
    return i.split("<")[0]


# ------------------------------------------------------------------------------------------------------ CPU: the gate
def built_instantiations(objects=FUSED_OBJECTS):
    """{demangled template id} of the kernels in the device objects `objects` (the fused path's), from their mangled symbols
    (_ZN4dpck12_GLOBAL__N_111k_gather_hwILi64ELi8ELi3EEEv... -> k_gather_hw<64, 8, 3>).  Only the dpck kernels count:
    k_zero_words (the memset kernel every object carries, dpc_common.h), the stage kernels (dpc_stages.o) and the nearest-point
    kernels (dpc_nearest.o) are not the fused path and are out of this gate's scope."""
    import re

    out = set()
    for obj in objects:
        for line in device_object_output(obj, ["llvm-readelf", "-sW"]).splitlines():
            f = line.split()
            if len(f) < 8 or f[3] != "FUNC":
                continue
            m = re.match(r"_ZN4dpck12_GLOBAL__N_1(\d+)(\w+)$", f[7])
            if not m:
                continue
            n = int(m.group(1))
            name, rest = m.group(2)[:n], m.group(2)[n:]
            targs = re.match(r"I((?:Li-?\d+E)+)E", rest)
            out.add(name + ("<%s>" % ", ".join(re.findall(r"Li(-?\d+)E", targs.group(1))) if targs else ""))
    return out


def test_matrix_names_every_instantiation_in_the_build():
    """The kernel symbols of the fused-path device objects == (what CASES claims) + UNREACHABLE, exactly."""
    built = built_instantiations()
    assert len(built) > 150, sorted(built)
    claimed = set().union(*(c.ids for c in CASES))
    assert not claimed & set(UNREACHABLE), "listed as unreachable and claimed by a row: %s" % sorted(claimed & set(UNREACHABLE))
    missing = sorted(built - claimed - set(UNREACHABLE))
    stale = sorted((claimed | set(UNREACHABLE)) - built)
    assert not missing, "instantiations no row of CASES launches (add a row, or an UNREACHABLE entry with its reason): %s" % missing
    assert not stale, "rows / UNREACHABLE entries naming instantiations the build does not contain: %s" % stale
    assert len({c.name for c in CASES}) == len(CASES)


def test_matrix_rows_ask_for_the_buckets_they_claim():
    """CPU check of the table itself: every row's kernels need the radius buckets its ids carry (dpc_taps_bucket), the
    ids of each row are consistent with its grid, and the radii are what the docstring promises (skewed kernels keep
    every tap)."""
    import dpc.render as R
    from oracle import dpc_oracle as O

    for c in CASES:
        cfg, kern = kernels(c, O)
        if kern is None:
            continue
        kx = kern[0].reshape(-1).numpy()
        kz = kern[2].reshape(-1).numpy()
        bx, bz = R.taps_bucket(kx), R.taps_bucket(kz)
        assert bx in BUCKETS, (c.name, bx)
        if not isinstance(c.rxy, tuple):
            assert not np.array_equal(kx, kx[::-1]) or c.rxy == 0, c.name + ": the x/y kernel is symmetric"
            assert kx.min() > 1e-4 * kx.sum() or c.rxy == 0, c.name
        for i in c.ids:
            args = [int(a) for a in i[i.index("<") + 1:-1].split(",")] if "<" in i else []
            fam = _family(i)
            if fam in ("k_splat_hw", "k_gather_hw"):
                assert args[2] == bx and args[0] in (0, c.G), (c.name, i, bx)
            elif fam == "k_splat_xl":
                assert args[1] == bx and c.G == 64, (c.name, i, bx)
            elif fam in ("k_zcol_fwd", "k_zcol_bwd", "k_zcol_fwdbwd"):
                assert args[0] == c.D and args[1] == bz, (c.name, i, bz)
            elif fam in ("k_zcol_fwd_dyn", "k_zcol_bwd_dyn"):
                assert bz == -1 or c.D not in (32, 64, 128), (c.name, i, bz)


# ------------------------------------------------------------------------------------------------------ GPU: the matrix
def _gt(S, G, seed):
    g = torch.Generator().manual_seed(seed)
    mask = (torch.rand(S, 1, 2 * G, 2 * G, generator=g) > 0.5).double()
    return torch.nn.AvgPool2d(2)(mask).permute(0, 2, 3, 1).contiguous()


def _dev(x, grad=False):
    if x is None:
        return None
    t = x.detach().to("cuda", torch.float32 if x.dtype != torch.float64 else torch.float64).contiguous()
    return t.requires_grad_(True) if grad else t


def _run_locate(c, R, O, cfg):
    B, N = c.B, c.N
    pc, q, _, _, _, _ = O.synth_inputs(B, N, 2, _seed(c))
    tr = O.pc_perspective_transform(cfg, pc, q).detach()      # fp64 (z, y, x), the reference's own direct-caller input
    tr = tr.float().double() if c.keep == "f32" else tr
    w = torch.rand(B, c.D, c.G, c.G, generator=torch.Generator().manual_seed(_seed(c) + 1), dtype=torch.float64)
    gtr = (tr.float() if c.keep == "f32" else tr).cuda().requires_grad_(True)
    from dpc.render import _native

    got = {}

    def device():
        vox, _ = R.pointcloud2voxels3d_fast(cfg, gtr)
        (vox * w.cuda().to(vox.dtype)).sum().backward()
        got["vox"] = vox.detach()

    ids = _native.launched_instantiations(device, torch.device("cuda"))
    ctr = tr.clone().requires_grad_(True)
    rvox, _ = O.pointcloud2voxels3d_fast(cfg, ctr)
    (rvox * w).sum().backward()
    close(got["vox"], rvox, TOL, "matrix %s: voxels" % c.name)
    close(gtr.grad, ctr.grad, TOL, "matrix %s: d(tr)" % c.name)
    return ids


def _run_projection(c, R, O, cfg, kern):
    from dpc.render import _native

    B, N, K, Rp, G = c.B, c.N, c.K, c.R, c.G
    S = B // K
    seed = _seed(c)
    pcs, _, _, _, _, _ = O.synth_inputs(B // Rp, N, 2, seed)
    _, q, s, _, t, f = O.synth_inputs(B, 4, 2, seed + 1, with_t=c.t, with_f=c.f)
    gt = _gt(S, G, seed + 2)
    w = torch.rand(B, G, G, 1, generator=torch.Generator().manual_seed(seed + 3), dtype=torch.float64)
    d = torch.device("cuda")
    idx = None
    if c.keep is not None:
        idx = R.point_dropout_indices(B, N, c.keep, d, torch.Generator(device="cuda").manual_seed(seed + 4))
    rkern = R.smoothing_kernel(cfg, c.rxy[1]) if isinstance(c.rxy, tuple) else kern
    gp, gq, gs, gtt, gf = _dev(pcs, True), _dev(q, True), _dev(s, True), _dev(t, True), _dev(f, True)
    got = {}

    def device():
        if c.path == "plain":
            out = R.pointcloud_project_fast(cfg, gp, gq, gtt, None, rkern, scaling_factor=gs, focal_length=gf, point_index=idx)
            (out["proj"] * w.to(d, torch.float32)).sum().backward()
            got.update(proj=out["proj"].detach())
        elif c.path == "fwd":
            with torch.no_grad():
                got.update(proj=R.pointcloud_project_fast(cfg, gp, gq, gtt, None, rkern, scaling_factor=gs, focal_length=gf)["proj"])
        elif c.path == "loss":
            loss, out, win = R.pointcloud_project_loss(cfg, gp, gq, gtt, None, rkern, scaling_factor=gs, focal_length=gf,
                                                       gt=_dev(gt).float(), num_candidates=K, point_index=idx)
            (1.5 * loss).backward()
            got.update(proj=out["proj"].detach(), loss=loss.detach(), win=win)
        else:  # step
            sched = None
            if c.sched:
                sched = R.DeviceSchedule(d, kern[0].reshape(-1).numpy(), kern[2].reshape(-1).numpy())
            plan = R.project_loss_step(cfg, rkern, B, N, d, schedule=sched, num_candidates=K, point_replicas=Rp)
            plan.run(gp.detach(), gq.detach(), gs.detach(), _dev(gt).float(), t=None if t is None else gtt.detach(),
                     f=None if f is None else gf.detach())
            got.update(proj=plan.proj, loss=plan.loss, win=plan.winner, dpc=plan.dpc, dq=plan.dq, ds=plan.ds,
                       dt=plan.dt if t is not None else None, df=plan.df if f is not None else None)
        if c.path in ("plain", "loss"):
            got.update(dpc=gp.grad, dq=gq.grad, ds=gs.grad, dt=None if t is None else gtt.grad, df=None if f is None else gf.grad)

    ids = _native.launched_instantiations(device, d)
    got = {k: (v.detach().clone() if isinstance(v, torch.Tensor) else v) for k, v in got.items()}

    # the oracle, on the materialised clouds of the checked samples
    sub = list(range(S)) if c.sub is None else c.sub
    assert Rp == 1 or c.sub is None, "subsets of shared point sets are not supported"
    clouds = torch.tensor([smp * K + k for smp in sub for k in range(K)])
    tag = "matrix %s: " % c.name

    def oracle(nudge=None):
        leaf = lambda x: None if x is None else x.clone().requires_grad_(True)
        cp = leaf(pcs if c.sub is None else pcs[clouds])
        cq, cs = leaf(q[clouds]), leaf(s[clouds])
        ct, cf = leaf(None if t is None else t[clouds]), leaf(None if f is None else f[clouds])
        mat = cp.repeat_interleave(Rp, dim=0) if Rp > 1 else cp
        if idx is not None:
            mat = mat.gather(1, idx.long().cpu().unsqueeze(-1).expand(-1, -1, 3))
        O.DRC_CLAMP_NUDGE = nudge
        try:
            ref = O.pointcloud_project_fast(cfg, mat, cq, ct, None, kern, scaling_factor=cs, focal_length=cf)
        finally:
            O.DRC_CLAMP_NUDGE = None
        out = dict(ref=ref, proj=ref["proj"].detach())
        if c.path == "fwd":
            return out
        if c.path == "plain":
            (ref["proj"] * w[clouds]).sum().backward()
        else:
            scale = 1.5 if c.path == "loss" else 1.0
            out["loss"], out["win"] = O.proj_loss_pose_candidates(gt[sub], ref["proj"], K)
            (scale * out["loss"] * len(sub) / S).backward()       # the batch loss divides by all S samples
        out.update(dpc=cp.grad, dq=cq.grad, ds=cs.grad, dt=None if ct is None else ct.grad, df=None if cf is None else cf.grad)
        return out

    ref = oracle()
    close(got["proj"][clouds.cuda()], ref["proj"], TOL, tag + "proj")
    if c.path == "fwd":
        return ids
    if c.path != "plain":
        assert np.array_equal(got["win"].cpu().numpy()[sub], ref["win"].numpy()), tag + "winners"
        if c.sub is None:
            close(got["loss"], ref["loss"], TOL, tag + "loss")
        else:   # the reference's formula on the device's own silhouettes (all samples)
            close(got["loss"], O.proj_loss_pose_candidates(gt, got["proj"].double().cpu(), K)[0], TOL, tag + "loss")
    grads = [("dpc", "d(points)", True)] + [(k, "d(%s)" % k[1], False) for k in ("dq", "ds", "dt", "df")]
    grads = [(k, what, per_set) for k, what, per_set in grads if ref[k] is not None]
    dev_grad = lambda k, per_set: got[k] if per_set and c.sub is None else got[k][clouds.cuda()]
    if c.clamp_flip:
        # Judged like tests/test_gpu_parity.py::test_drc_clamp_threshold_flip_is_bounded_and_explained.  The fused kernels
        # run the taps plan_taps keeps (outer taps worth < 1e-8 of the kernel's mass dropped, csrc/dpc_kernels.h): the same
        # fp64 forward with THOSE taps names the voxels that the drop moves across the DRC clamp's eps / 1 - eps (drc.py:57).
        # They must be few and each within 1e-3 relative of its threshold; forcing the oracle to the dropped-tap decision
        # there (O.DRC_CLAMP_NUDGE, invisible to every forward value) must explain every gradient by the rule.
        eps = cfg.drc_logsum_clip_val
        v = ref["ref"]["voxels"].detach()
        mat = pcs if c.sub is None else pcs[clouds]
        mat = mat.repeat_interleave(Rp, dim=0) if Rp > 1 else mat
        dv = O.pointcloud_project_fast(cfg, mat, q[clouds], None if t is None else t[clouds], None, [_planned(k) for k in kern],
                                       scaling_factor=s[clouds], focal_length=None if f is None else f[clouds])["voxels"]
        passes = lambda x: (x >= eps) & (x <= 1.0 - eps)
        flipped = (passes(v) != passes(dv)).nonzero().tolist()
        assert 1 <= len(flipped) <= 8, tag + "%d voxels that the tap drop moves across the clamp" % len(flipped)
        nudge = torch.zeros_like(v)
        for b, z, y, x, _ in flipped:
            val = v[b, z, y, x, 0].item()
            th = eps if abs(val - eps) <= abs(val - (1.0 - eps)) else 1.0 - eps
            assert abs(val - th) <= 1e-3 * th, tag + "voxel %s is %.3e relative from its threshold" % ((b, z, y, x), abs(val - th) / th)
            inside = (1.0 + 1e-9) if th == eps else (1.0 - 1e-9)
            nudge[b, z, y, x, 0] = th * (inside if not passes(v[b, z, y, x, 0]) else 2.0 - inside) - val
        for k, what, per_set in grads:    # the un-nudged distance, reported (the explained event; not a bound)
            a, r = dev_grad(k, per_set).double().cpu(), ref[k].double()
            ERRORS.append((tag + what + " vs the UN-NUDGED oracle (%d flipped voxels; not a bound)" % len(flipped),
                           float((a - r).abs().max()), max(1.0, float(r.abs().max()))))
        ref = oracle(nudge)
        assert (ref["proj"] - oracle()["proj"]).abs().max().item() < 1e-9, tag + "the nudge shows in the forward"
        tag += "nudged to the device's clamp decisions: "
    for k, what, per_set in grads:
        close(dev_grad(k, per_set), ref[k], TOL, tag + what)
    return ids


@pytest.fixture(scope="module")
def O():
    from oracle import dpc_oracle as O

    O.EXACT_POSE_GRADIENT = True   # d(q) against the exact fp64 sum over the points, as tests/test_gpu_parity.py does
    yield O
    O.EXACT_POSE_GRADIENT = False


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_instantiation_vs_oracle(O, c):
    import dpc.render as R

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    cfg, kern = kernels(c, O)
    ids = _run_locate(c, R, O, cfg) if c.path == "locate" else _run_projection(c, R, O, cfg, kern)
    assert c.ids <= ids, "%s: the launchers picked %s, the row expects %s (missing %s)" % (
        c.name, sorted(ids), sorted(c.ids), sorted(c.ids - ids))


@pytest.mark.gpu
def test_zz_matrix_error_report():
    """Not a check: rewrites the suite's margin report (tests/test_gpu_parity.py::test_zz_error_report) so that it holds this
    module's comparisons too -- they go into the same ERRORS list, after that module's report was written."""
    import test_gpu_parity

    assert any(what.startswith("matrix ") for what, _, _ in ERRORS)
    test_gpu_parity.test_zz_error_report()
