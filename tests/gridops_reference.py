"""Plain float64 reference of the grid operators' box kernels (csrc/sdfk_gridops.inc), and the shapes they are tested on.

scipy.ndimage.convolve(u, ones(ks)) with mode="reflect" is, per axis, a window over the offsets -((k-1)//2) .. k//2 of
the symmetrically extended array; np.pad(mode="symmetric") reflects repeatedly when the pad is wider than the array,
which is what sdfk_reflect does.

Why a bit-exact comparison is possible: the kernels accumulate in float64 and round to fp32 once. On inputs of the form
m * 2**-12 with integer |m| < 2**20 (`dyadic`) every partial sum of up to 2**20 taps is a multiple of 2**-12 below
2**28 — exact in float64 in ANY order — and what follows, one float64 product with 1.0 / (k0*k1*k2) and one cast to
fp32, numpy performs identically. So the reference neither needs a tolerance nor has to copy a summation order, and it
may sum axis by axis (k0 + k1 + k2 shifted views instead of k0*k1*k2).
"""
import numpy as np


def box_sum(u, ks):
    """Sum over the ks window around every point of the reflected field, float64."""
    acc = np.asarray(u, dtype=np.float64)
    assert acc.ndim == len(ks)
    for axis, k in enumerate(ks):
        k, n = int(k), acc.shape[axis]
        pad = [(0, 0)] * acc.ndim
        pad[axis] = ((k - 1) // 2, k // 2)
        ext = np.pad(acc, pad, mode="symmetric")
        acc = np.zeros_like(acc)
        for tap in range(k):
            acc += np.take(ext, range(tap, tap + n), axis=axis)
    return acc


def taps(ks):
    return int(np.prod([int(k) for k in ks]))


def box_average64(u, ks):
    """The average before its rounding to fp32: the product is formed in float64, as in sdfk_grid_box_average."""
    return box_sum(u, ks) * (1.0 / float(taps(ks)))


def box_average(u, ks):
    return box_average64(u, ks).astype(np.float32)


def edge_kernel(ndim):
    return (3, 3) if ndim == 2 else (3, 3, 1)


def edge_detect64(u):
    u = np.asarray(u, dtype=np.float64)
    return 9.0 * u - box_sum(u, edge_kernel(u.ndim))


def edge_detect(u):
    return edge_detect64(u).astype(np.float32)


def dyadic(rng, shape):
    """fp32 noise m * 2**-12, integer |m| < 2**20: every sum of up to 2**20 of them is exact in float64."""
    m = rng.integers(-(2 ** 20) + 1, 2 ** 20, size=shape)
    return (m.astype(np.float64) * 2.0 ** -12).astype(np.float32)


# ---- what the box dispatch can do, and the cases that reach all of it -------------------------------------------------
def dims3(shape):
    return tuple(shape) + (1,) * (3 - len(shape))


def variant_names(shape, ks, out8):
    """Names of the dispatch features a launch on `shape` with kernel `ks` shows, from sdfk_debug_box_variant's out8
    (include/sdfk.h) and the arguments."""
    flags, k0c, k2c, pc, chunks, gx, gy, gz = (int(v) for v in out8)
    march, fast, flat = bool(flags & 1), bool(flags & 2), bool(flags & 4)
    n = dims3(shape)
    k = dims3(ks)
    if flat:                                                   # the kernels' view of a flat field
        n, k = (1, n[0], n[1]), (1, k[0], k[1])
    kt = (n[2] + 63) // 64
    names = set()
    if march:
        names |= {"march K0C=%d" % k0c, "march K2C=%d" % k2c}
        if gz > 1:
            names.add("march: several segments")
        if gy > 1:
            names.add("march: several j tiles")
        if gx > 1:
            names.add("march: several k tiles")
    else:
        names.add("tiled FAST K2C=%d" % k2c if fast else "tiled FAST=false")
        if k[0] == 6:
            names.add("tiled because k0 = 6")
        if k[0] > 7:
            names.add("tiled because k0 > 7")
        if fast and k[0] <= 7 and k[0] != 6:
            names.add("tiled because the halo tile is too wide")
        if chunks > 1:
            names.add("tiled: several LDS chunks")
        if gx < kt:
            names.add("tiled: walk along k")
        if gy > 1:
            names.add("tiled: several j tiles")
        if kt > 1:
            names.add("tiled: several k tiles")
    if flat:
        names.add("flat relabelling")
    return names


ALL_VARIANTS = ({"march K0C=%d" % k for k in (1, 2, 3, 4, 5, 7)} | {"march K2C=%d" % k for k in (1, 3, 5, 0)}
                | {"tiled FAST K2C=%d" % k for k in (1, 2, 3, 4, 5, 7, 0)}
                | {"tiled FAST=false", "tiled because k0 = 6", "tiled because k0 > 7", "tiled because the halo tile is too wide",
                   "tiled: several LDS chunks", "tiled: walk along k", "tiled: several j tiles", "tiled: several k tiles",
                   "march: several segments", "march: several j tiles", "march: several k tiles", "flat relabelling"})

# (33, 9, 65): a segment seam (32 planes), j tiles of 8 (marching) and 4 (tiled) rows that are not full, two k tiles with
#              the last point alone in its tile
# (5, 13, 130): the last row alone in its j tile (tiled), half a thread's row pair missing (marching), three k tiles
# (32, 8, 64): exactly full tiles, nothing masked
_SEAMS = (33, 9, 65)
_ROWS = (5, 13, 130)
_FULL = (32, 8, 64)
# (6, 2, 2) and (8, 3, 5) are here for the tiled kernel's K2C = 2 and 5 instances: with k0 <= 7 (other than 6) and a
# narrow tile those k2 belong to the marching kernel
_KERNELS = ((3, 3, 3), (2, 4, 6), (4, 2, 1), (5, 5, 5), (7, 7, 7), (1, 1, 2), (1, 3, 1),
            (6, 3, 3), (8, 1, 4), (9, 9, 9), (3, 8, 7), (2, 2, 7), (11, 3, 1), (6, 2, 2), (8, 3, 5))
CASES = (
    [(_SEAMS, k) for k in _KERNELS]
    + [(_ROWS, k) for k in ((3, 3, 3), (5, 5, 5), (2, 4, 6), (6, 3, 3), (8, 1, 4), (9, 9, 9), (3, 8, 7))]
    + [(_FULL, k) for k in ((3, 3, 3), (7, 7, 7), (2, 4, 6), (6, 3, 3), (9, 9, 9))]
    # degenerate grids; with n2 = 1 the host folds k2 away, so k2 = 1 or a power-of-two product (both scalings exact)
    + [((1, 1, 1), (3, 3, 1)), ((1, 1, 1), (2, 2, 2)),
       ((2, 2, 2), (3, 3, 3)), ((2, 2, 2), (5, 5, 5)), ((2, 2, 2), (2, 4, 6)), ((2, 2, 2), (7, 7, 7)),
       ((1, 7, 3), (3, 3, 3)), ((1, 7, 3), (1, 3, 1)), ((1, 7, 3), (5, 5, 5)),
       ((3, 1, 70), (3, 3, 3)), ((3, 1, 70), (6, 3, 3)), ((3, 1, 70), (2, 4, 6)),
       ((70, 3, 1), (4, 2, 1)), ((70, 3, 1), (2, 4, 2)), ((70, 3, 1), (11, 3, 1))]
    # kernels wider than the field: reflections of reflections (FAST = false)
    + [((3, 2, 5), (9, 7, 13)), ((1, 1, 4), (5, 5, 5)), ((3, 2, 5), (3, 8, 7))]
    # n0 * ceil(n1 / 4) >= 16384 rows: one workgroup per row block walks both k tiles
    + [((128, 512, 65), (6, 3, 3))]
    # flat fields, relabelled (1, n0, n1)
    + [((77, 130), k) for k in ((3, 3), (2, 4), (5, 5), (7, 7), (9, 9), (8, 7))]
    + [((300, 2), k) for k in ((3, 3), (4, 2), (11, 3))]
)
BIG = (128, 512, 65)
