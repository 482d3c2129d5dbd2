"""The bit-reproducible colour splat without a GPU: the C ABI's bookkeeping (header, exports, binding), the refusals of its
entry points, which need no device, and the refusals and the config key of the Python surface."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dpc_render.h")
NEW_SYMBOLS = ("dpc_rgb_splat_fixed_workspace_bytes", "dpc_rgb_splat_fixed_fwd", "dpc_rgb_splat_fixed_bwd")


def test_header_exports_and_binding_agree():
    from dpc.render import _native

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = {m.group(2): (m.group(1), m.group(3))
              for m in re.finditer(r"\b(\w+)\s+(dpc_rgb_splat_fixed_\w+)\s*\(([^;]*?)\)\s*;", text)}
    assert sorted(protos) == sorted(NEW_SYMBOLS)
    exported = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    L = _native.lib()
    assert L.dpc_abi_version() == 15 == _native.ABI_VERSION
    ctype = {"int32_t": ctypes.c_int32, "uint64_t": ctypes.c_uint64}
    for name in NEW_SYMBOLS:
        assert name in _native.SYMBOLS and name in exported
        ret, args = protos[name]
        fn = getattr(L, name)
        assert ctypes.sizeof(fn.restype) == ctypes.sizeof(ctype[ret]), name
        want = []
        for a in (x.strip() for x in args.split(",")):
            if a.startswith("const DpcParams*"):
                want.append(ctypes.POINTER(_native.DpcParams))
            elif "*" in a:
                want.append(ctypes.c_void_p)
            else:
                want.append(ctype[a.split()[0]])
        assert [ctypes.sizeof(t) for t in fn.argtypes] == [ctypes.sizeof(t) for t in want], name
        assert [t is ctypes.c_void_p for t in fn.argtypes] == [t is ctypes.c_void_p for t in want], name
    # the first colour entry points are what they were: they keep refusing shared sets
    P = _native.DpcParams(4, 10, 8, 8, 8, 0, 0, 2.0, 1.875, 1e-5, 10.0, 2, 0, None, None, None, None, None)
    one = ctypes.c_void_p(256)
    assert L.dpc_rgb_splat_fwd(ctypes.byref(P), one, one, one, None) == _native.DPC_ERR_SHAPE


def test_refusals_come_before_any_device_call():
    """Every call below is refused on its arguments (the pointers are never dereferenced), or has nothing to do."""
    from dpc.render import _native

    L = _native.lib()
    SHAPE, NULL = _native.DPC_ERR_SHAPE, _native.DPC_ERR_NULL
    one = ctypes.c_void_p(256)
    fwd, bwd, size = L.dpc_rgb_splat_fixed_fwd, L.dpc_rgb_splat_fixed_bwd, L.dpc_rgb_splat_fixed_workspace_bytes

    def params(B=4, N=10, R=1, n_src=0, index=None, n_live=None, D=8):
        return _native.DpcParams(B, N, D, 8, 8, 0, 0, 2.0, 1.875, 1e-5, 10.0, R, n_src, index, None, n_live, None, None)

    P = params()
    ref = ctypes.byref(P)
    # sizes: 8 bytes per colour voxel and 4 per cloud, rounded up to 256; nothing for the gradient without sharing
    assert size(ref, 10) == (4 * 3 * 512 * 8 + 4 * 4 + 255) // 256 * 256
    assert size(ctypes.byref(params(B=4, R=2)), 10) == size(ref, 10)             # the sets' sums are the smaller part here
    big_sets = params(B=4, N=10, R=2, n_src=100000, index=256)
    assert size(ctypes.byref(big_sets), 100000) == (2 * 100000 * 3 * 8 + 2 * 4 + 255) // 256 * 256   # ... and the larger here
    assert size(ref, 9) == 0 and size(None, 10) == 0                              # invalid arguments
    # null pointers
    assert fwd(None, one, one, 10, one, one, None) == NULL and bwd(None, one, one, 10, one, one, one, one, None) == NULL
    for args in ((None, one, one, one), (one, None, one, one), (one, one, None, one), (one, one, one, None)):
        tr, rgb, out, ws = args
        assert fwd(ref, tr, rgb, 10, out, ws, None) == NULL, args
    for args in ((None, one, one, one), (one, None, one, one), (one, one, None, one), (one, one, one, None)):
        tr, rgb, dC, drgb = args
        assert bwd(ref, tr, rgb, 10, dC, drgb, None, None, None) == NULL, args
    shared = params(B=4, R=2)
    assert bwd(ctypes.byref(shared), one, one, 10, one, one, one, None, None) == NULL     # shared sets need the workspace
    # shapes
    for bad, n_set in ((params(n_live=256), 10),              # the colour step is not capturable
                       (params(B=5, R=2), 10),                # B % R != 0
                       (params(), 0), (params(), -1),         # n_set < 1
                       (params(), 11),                        # no index: a set is the cloud's own N colours
                       (params(n_src=20, index=256), 0),      # an index into nothing
                       (params(n_src=20, index=256), 21),     # n_set is the stored set's size
                       (params(D=2000), 10)):
        r = ctypes.byref(bad)
        assert fwd(r, one, one, n_set, one, one, None) == SHAPE, (n_set,)
        assert bwd(r, one, one, n_set, one, one, one, one, None) == SHAPE, (n_set,)
        assert size(r, n_set) == 0
    # shape errors win over null pointers (they are checked first)
    assert fwd(ctypes.byref(params(n_live=256)), None, None, 10, None, None, None) == SHAPE
    # no clouds: nothing to do, pointers may be null
    empty = params(B=0)
    assert fwd(ctypes.byref(empty), None, None, 10, None, None, None) == 0
    assert bwd(ctypes.byref(empty), None, None, 10, None, None, None, None, None) == 0


def _outputs(S=4, n=5, G=8):
    import dpc.render as R

    return R.ProjectionOutputs(torch.zeros(S, G, G, 1), lambda: {"tr_pc": torch.zeros(S, n, 3), "voxels": torch.zeros(S, G, G, G, 1)})


def test_value_errors_of_the_python_surface():
    import dpc.render as R
    from dpc.harness.config import chair_unsupervised

    off, on = chair_unsupervised(vox_size=8), chair_unsupervised(vox_size=8, pc_rgb_deterministic=True)
    images = torch.zeros(4, 8, 8, 3)
    sets, per_cloud = torch.zeros(2, 5, 3), torch.zeros(4, 5, 3)
    index = torch.zeros(4, 5, dtype=torch.int32)
    # without the key: sets and a point_index are refused, and the message says what to do
    for call in (lambda: R.proj_rgb_loss(off, _outputs(), sets, images),
                 lambda: R.rgb_grids(off, _outputs(), per_cloud, point_index=index),
                 lambda: R.project_rgb(off, _outputs(), torch.zeros(2, 9, 3), point_index=index),
                 lambda: R.drc_rgb_loss(off, _outputs(), sets, images, point_index=index)):
        with pytest.raises(ValueError, match="replicate_rgb") as e:
            call()
        assert "pc_rgb_deterministic" in str(e.value) and "all_rgb must hold" in str(e.value)
    # with the key: a point_index of the wrong shape
    for bad in (torch.zeros(4, 6, dtype=torch.int32), torch.zeros(2, 5, dtype=torch.int32), torch.zeros(20, dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"point_index must be \[4, 5\]"):
            R.rgb_grids(on, _outputs(), torch.zeros(2, 9, 3), point_index=bad)
    # ... and colours that are neither per cloud nor sets
    for bad, idx in ((torch.zeros(2, 4, 3), None),      # sets without an index must hold n colours
                     (torch.zeros(3, 5, 3), None),      # 4 clouds cannot share 3 sets
                     (torch.zeros(3, 9, 3), index),
                     (torch.zeros(4, 5), None), (torch.zeros(4, 5, 4), None), (torch.zeros(8, 5, 3), None)):
        with pytest.raises(ValueError, match="all_rgb must hold one colour per projected point.*colour sets"):
            R.proj_rgb_loss(on, _outputs(), bad, images, point_index=idx)
    # valid layouts pass the host checks and stop at the device check (there is no CPU path)
    for rgb, idx in ((per_cloud, None), (sets, None), (torch.zeros(2, 9, 3), index), (torch.zeros(1, 9, 3), index)):
        with pytest.raises(RuntimeError, match="MI355X"):
            R.rgb_grids(on, _outputs(), rgb, point_index=idx)
    from dpc.render._ops import colour_sets

    assert colour_sets((4, 5, 3), (4, 5, 3)) == 1 and colour_sets((4, 5, 3), (2, 5, 3)) == 2
    assert colour_sets((4, 5, 3), (1, 9, 3), index) == 4 and colour_sets((0, 5, 3), (0, 5, 3)) == 1


def test_key_defaults_to_false():
    from dpc.harness.config import chair_unsupervised

    cfg = chair_unsupervised()
    assert cfg.pc_rgb_deterministic is False and cfg["pc_rgb_deterministic"] is False
    assert chair_unsupervised(pc_rgb_deterministic=True).pc_rgb_deterministic is True
