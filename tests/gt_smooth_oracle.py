"""fp64 numpy restatement of the ground-truth node (csrc/dpc_gt_smooth.hip, dpc.render.smooth_gt): remap, resize by an
integer factor, and gauss_smoothen_image's two zero-padded passes (dpc/util/gauss_kernel.py:14-24: tf.nn.depthwise_conv2d
with a [1,fsz] kernel, then with a [fsz,1] kernel, padding "SAME", the same taps for every channel).

Everything works on [S,C,Hs,Ws] planes and returns [S,H,W,C], the layout the reference has after its permute."""
import numpy as np


def planes(gt, channels, planar):
    """[S,C,Hs,Ws] fp64 from [S,C,Hs,Ws] (planar) or [S,Hs,Ws,C]."""
    g = np.asarray(gt, dtype=np.float64)
    if g.ndim == 3:
        g = g[:, None]
    elif not planar:
        g = np.moveaxis(g, 3, 1)
    assert g.ndim == 4 and g.shape[1] == channels, (g.shape, channels)
    return g


def remap(g, remap_from, remap_to):
    return g if remap_from == remap_to else np.where(g == remap_from, remap_to, g)


def resize(g, f, mode):
    """mode "mean": the f x f average of nn.AvgPool2d(f); "sample": g[..., f*y, f*x]."""
    S, C, Hs, Ws = g.shape
    assert Hs % f == 0 and Ws % f == 0
    if mode == "sample":
        return g[:, :, ::f, ::f]
    assert mode == "mean"
    return g.reshape(S, C, Hs // f, f, Ws // f, f).mean(axis=(3, 5))


def blur_axis(g, taps, axis):
    """out[i] = sum_t taps[t] g[i + t - c], c = (n - 1) / 2, zeros outside: depthwise_conv2d is a correlation, "SAME" pads an
    odd kernel by c on both sides."""
    taps = np.asarray(taps, dtype=np.float64).reshape(-1)
    n = taps.size
    assert n % 2 == 1
    c = n // 2
    pad = [(0, 0)] * g.ndim
    pad[axis] = (c, c)
    gp = np.pad(g, pad)
    out = np.zeros_like(g)
    L = g.shape[axis]
    for t in range(n):
        out += taps[t] * np.take(gp, np.arange(t, t + L), axis=axis)
    return out


def blur(g, taps):
    """Rows first ([1,fsz]: along x), then columns ([fsz,1]: along y)."""
    return blur_axis(blur_axis(g, taps, 3), taps, 2)


def smooth_gt(gt, channels, planar, f, mode, taps, remap_from=0.0, remap_to=0.0):
    g = resize(remap(planes(gt, channels, planar), remap_from, remap_to), f, mode)
    return np.ascontiguousarray(np.moveaxis(blur(g, taps), 1, 3))


def resized_only(gt, channels, planar, f, mode, remap_from=0.0, remap_to=0.0):
    g = resize(remap(planes(gt, channels, planar), remap_from, remap_to), f, mode)
    return np.ascontiguousarray(np.moveaxis(g, 1, 3))


def gauss_kernel_1d(l, sig):
    """dpc/util/gauss_kernel.py:5-11 in fp64 (the fixture holds the reference's own fp32 taps)."""
    x = np.arange(-l // 2 + 1.0, l // 2 + 1)
    k = np.exp(-x ** 2 / (2.0 * sig ** 2))
    return k / k.sum()
