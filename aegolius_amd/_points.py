"""`Points.to_image` on the GPU (kernels: csrc/sdfk_points.inc).

The reference bins the cloud with `numpy.histogramdd(cloud.T, bins, range)`, keeps `count > 0` as float64 and extends
the occupied region plane by plane. Here the inputs are checked and the bin edges built on the host exactly as numpy
does (same exceptions, `numpy.linspace` edges); the occupancy grid is one byte per voxel in HBM, binned, extended and
widened there. Only the edge tables, the cloud, rx + ry + rz plane flags and the result cross PCIe.
"""
import contextlib
import ctypes
import operator

import numpy as np

from . import _engine
from .cores.helper_functions import resolution_conversion

_AXIS = {"X": 0, "Y": 1, "Z": 2}

# how the host result crosses PCIe: "bytes" = 1 B/voxel, widened to float64 on the host; "f64" = widened on the device,
# 8 B/voxel (DESIGN.md 4.12 has both measured)
DEFAULT_TRANSFER = "bytes"


def _outer_edges(first_edge, last_edge):
    """numpy's outer-edge rule for an explicit range (numpy/lib/_histograms_impl.py, _get_outer_edges)."""
    if first_edge > last_edge:
        raise ValueError("max must be larger than min in range parameter.")
    if not (np.isfinite(first_edge) and np.isfinite(last_edge)):
        raise ValueError("supplied range of [{}, {}] is not finite".format(first_edge, last_edge))
    if first_edge == last_edge:
        first_edge = first_edge - 0.5
        last_edge = last_edge + 0.5
    return first_edge, last_edge


def prepare(cloud, co_size, co_resolution, extend):
    """Everything of to_image that needs no GPU, in the reference's order: the converted resolution, then the checks of
    numpy.histogramdd and its edges. Returns (sample (3, N) float64 C-contiguous, res, edges, extend entries)."""
    res = (resolution_conversion(co_resolution[0]), resolution_conversion(co_resolution[1]),
           resolution_conversion(co_resolution[2]))
    ranges = ((-co_size[0] / 2, co_size[0] / 2), (-co_size[1] / 2, co_size[1] / 2), (-co_size[2] / 2, co_size[2] / 2))
    sample = np.asarray(cloud).T
    try:
        n, d = sample.shape
    except (AttributeError, ValueError):
        sample = np.atleast_2d(sample).T
        n, d = sample.shape
    if len(res) != d:
        raise ValueError("The dimension of bins must be equal to the dimension of the sample x.")
    edges = []
    for i in range(3):
        if res[i] < 1:
            raise ValueError("`bins[{}]` must be positive, when an integer".format(i))
        lo, hi = _outer_edges(*ranges[i])
        edges.append(np.linspace(lo, hi, operator.index(res[i]) + 1))
    entries = list(extend)
    return np.ascontiguousarray(sample.T, dtype=np.float64), res, edges, entries


def _plane_range(flags, sign):
    """(source plane, lo, hi) of one extend step, numpy's IndexError on an axis without an occupied plane."""
    occupied = np.flatnonzero(flags)
    if occupied.size == 0:
        raise IndexError("index %d is out of bounds for axis 0 with size 0" % (0 if sign == "-" else -1))
    if sign == "-":
        src = int(occupied[0])
        return src, 0, src
    src = int(occupied[-1])
    return src, src + 1, flags.size


def to_image(cloud, co_size, co_resolution, extend, resident=False, device=0, transfer=None, timings=None):
    """The reference's Points.to_image grid: (rx, ry, rz) float64 on the host, or (resident=True) a DeviceField of
    rx ry rz float32 0 / 1 values in C order. `transfer`: "bytes" or "f64" (see DEFAULT_TRANSFER). `timings`: a dict
    that receives device-event milliseconds of the phases bin / extent / fill / transfer."""
    sample, res, edges, entries = prepare(cloud, co_size, co_resolution, extend)
    transfer = transfer or DEFAULT_TRANSFER
    if transfer not in ("bytes", "f64"):
        raise ValueError("transfer must be 'bytes' or 'f64'")
    _engine.require_gpu()
    L = _engine.lib()
    _engine.check(L.sdfk_set_device(int(device)), "sdfk_set_device")
    rx, ry, rz = res
    nvox = rx * ry * rz
    n = sample.shape[1]
    table = np.ascontiguousarray(np.concatenate(edges), dtype=np.float64)
    timer = _engine.Timer(timings)
    with contextlib.ExitStack() as on_error, contextlib.ExitStack() as stack:
        def alloc(nbytes):
            return stack.enter_context(_engine.DeviceBuffer(nbytes, what="to_image"))
        grid = alloc(nvox)
        d_grid = grid.at()
        d_edges = alloc(table.nbytes)
        d_edges.upload(table)
        d_cloud = None
        if n:
            cloud_buf = alloc(sample.nbytes)
            cloud_buf.upload(sample)
            d_cloud = cloud_buf.at()
        timer.mark("start")
        _engine.check(L.sdfk_points_bin(d_cloud, n, n, d_edges.at(), rx, ry, rz, d_grid, None), "sdfk_points_bin")
        timer.mark("bin")
        steps = [(ex[0], _AXIS[ex[1]]) for ex in entries if ex in ("-X", "+X", "-Y", "+Y", "-Z", "+Z")]
        if steps:
            d_flags = alloc(rx + ry + rz)
            _engine.check(L.sdfk_points_extent(d_grid, rx, ry, rz, d_flags.at(), None), "sdfk_points_extent")
            flags = d_flags.download(np.empty(rx + ry + rz, dtype=np.uint8))
            timer.mark("extent")
            per_axis = [flags[:rx], flags[rx:rx + ry], flags[rx + ry:]]
            for sign, axis in steps:
                src, lo, hi = _plane_range(per_axis[axis], sign)
                if hi > lo:
                    _engine.check(L.sdfk_points_fill(d_grid, rx, ry, rz, axis, src, lo, hi, None), "sdfk_points_fill")
                    per_axis[axis][lo:hi] = 1          # a copied plane is occupied; the other axes' flags stay
            timer.mark("fill")
        if resident:
            field = on_error.enter_context(_engine.DeviceField(nvox, device))
            _engine.check(L.sdfk_points_widen(d_grid, nvox, 1, ctypes.c_void_p(field.ptr), None), "sdfk_points_widen")
            _engine.check(L.sdfk_sync(None), "sdfk_sync")
            timer.mark("transfer")
            timer.finish()
            on_error.pop_all()
            return field
        out = np.empty(res, dtype=np.float64)
        if transfer == "f64":
            d_wide = alloc(nvox * 8)
            _engine.check(L.sdfk_points_widen(d_grid, nvox, 0, d_wide.at(), None), "sdfk_points_widen")
            d_wide.download(out)
        else:
            np.copyto(out, grid.download(np.empty(res, dtype=np.uint8)), casting="safe")
        timer.mark("transfer")
        timer.finish()
        return out
