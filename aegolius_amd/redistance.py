"""Redistancing: the signed Euclidean distance of every grid point to a level set of a field (kernels:
csrc/sdfk_redistance.inc).

    from aegolius_amd import redistance
    d = redistance.redistance(field, (x, y, z))                  # (N,) float32, generate_grid's layout (z fastest)
    d = redistance.from_geometry(geometry, (2, 2, 2), (257, 257, 257), band=0.1)

Smooth unions, twist, bend, scaling, the falloff maps and every custom callable return a field with the right zero set and
the wrong metric. This takes any field, keeps its level set and returns a field with |grad| = 1: what `rounding`, `onion`,
the falloff widths, a mesh offset `isosurface(d, level=r)` and a Lipschitz bound of 1 need. The level set is the vertex set
of mesh.isosurface / mesh.contour of the same field; the distance is the distance to those points.

The definition (one definition: this text, the kernels and tests/redistance_reference.py). All arithmetic is float32,
every operation rounded once, in the order written.

 1. Inside, edges, seeds: mesh's rule. A point is inside iff f <= level; NaN is outside. Point (i, j, k) owns its +x, +y
    and +z edges. An edge whose ends differ in the inside test carries one seed at xa + t (xb - xa), t = (level - fa) /
    (fb - fa), a the lower end; if one end is NaN the seed is put at the other end; the other coordinates are the axis
    values. The seeds of the edges along axis a are family a. (A seed whose position is NaN — an infinite field value at an
    end of a crossing edge can give one, as it gives the mesh a NaN vertex — is dropped.)
 2. Squared distance per family, the family's own axis first and the other axes after it in increasing order (x: x y z,
    y: y x z, z: z x y; 2-D: x: x y, y: y x). Pass 1, along the family's axis, per grid line:
        g(i) = min over the line's seeds s of (x_i - s) (x_i - s),         +inf for a line without a seed
    and every further pass, along an axis b, is a min-plus pass:
        g'(j) = min over j' of g(j') + (b_j - b_j') (b_j - b_j')
    Q = the min over the families. A min over fixed float32 expressions does not depend on the order of evaluation and
    rounding is monotone, so this equals the brute-force min over all seeds of the family's expression, bit for bit. The
    device searches outward from every point and stops a side at the first source with d d >= best; no lower envelope of
    parabolas is built (it would choose winners by computed intersections and change bits).
 3. D = sqrt(Q), correctly rounded. With a `band`, D = min(D, float32(band)); each pass then looks only at sources within
    `band` along its axis, which cannot change min(D, band). Without any seed D = +inf, or `band`.
 4. Near band (near="gradient" only). At every point that is an end of a crossing edge, per axis of at least 2 points
        g_a = (f+ - f-) / (a+ - a-)      the neighbours on both sides; at the ends of an axis the one-sided difference
        m = sqrt((gx gx + gy gy) + gz gz)          (2-D: sqrt(gx gx + gy gy))
        e = |f - level| / m
    D = min(e, D) if every field value used, m, |f - level| and e are finite and m > 0; otherwise the point keeps D.
    The distance to the edge crossings alone overestimates in the first ring of points — by a factor sqrt(2) beside a
    plane at 45 degrees — and that moves the level set of the output; the first-order estimate keeps it to second order.
    The min guards against fields that are not smooth (sign fields, binarisations), where e is far too large.
 5. out = -D where inside, +D elsewhere. (A NaN point is outside: it comes out positive.)

`stats` receives `seeds` (int: the number of seeds, the vertex count of the mesh) and `ms` (dict: device-event
milliseconds per pass, named by the axes they ran along — "x", "xy", "y", "yx", "xyz", "z", "zx", "zxy" — and "finish").
Memory: the field, the output and 2 N floats of scratch.
"""
import ctypes

import numpy as np

from . import _engine
from .mesh import _is_geometry, _level, _grid_of, _points, _tables

NEAR = ("seeds", "gradient")
PASSES_3D = ("x", "xy", "y", "yx", "xyz", "z", "zx", "zxy", "finish")
PASSES_2D = ("x", "xy", "y", "yx", "finish")


def _axes(axes):
    """-> float32 tables (2 or 3) by mesh's rules: three tables, two, the three of a 2-D grid, or a tagged array."""
    tagged = getattr(axes, "grid_axes", None)
    given = tagged if tagged is not None else axes
    if tagged is None and isinstance(axes, np.ndarray) and axes.ndim == 2 and axes.shape[0] == 3:
        _tables(axes, 3)                                       # (raises: an untagged generate_grid array)
    given = [np.asarray(a).ravel() for a in given]
    flat = len(given) == 2 or (len(given) == 3 and given[2].size == 1 and given[2][0] == 0.0)
    return _tables(axes, 2 if flat else 3)


def _band(band):
    if band is None:
        return 0.0
    b = np.float32(band)
    if not (np.isfinite(b) and b > 0):
        raise ValueError("band must be finite and positive (or None); got %r" % (band,))
    return float(b)


def _near(near):
    if near not in NEAR:
        raise ValueError("near is one of %r; got %r" % (NEAR, near))
    return NEAR.index(near)


def field_redistance(d_field, tables, level, band, near, d_out, stats=None):
    """sdfk_field_redistance on device pointers (ints): the field and the output, each of prod(len(t) for t in tables)
    floats; scratch is allocated here. -> the number of seeds."""
    L = _engine.lib()
    ax, tab = _engine.axis_args(list(tables) + ([np.zeros(1, dtype=np.float32)] if len(tables) == 2 else []))
    shape = [a.size for a in ax]
    seeds = ctypes.c_int64(0)
    ms = (ctypes.c_float * 9)() if stats is not None else None
    with _engine.DeviceBuffer(max(L.sdfk_field_redistance_scratch(*shape), 8), what="redistance") as scratch:
        _engine.check(L.sdfk_field_redistance(ctypes.c_void_p(d_field), *tab, level, band, near, ctypes.c_void_p(d_out),
                                              scratch.at(), ctypes.byref(seeds), ms, None), "sdfk_field_redistance")
    if stats is not None:
        stats["seeds"] = seeds.value
        stats["ms"] = dict(zip(PASSES_2D if len(tables) == 2 else PASSES_3D, [float(v) for v in ms]))
    return seeds.value


def redistance(field, axes, level=0.0, band=None, near="gradient", resident=False, stats=None):
    """Signed distance to {field = level} on the grid of `axes` (see the module text) -> (N,) float32, or a DeviceField
    with resident=True. `field`: a DeviceField (left unchanged), a host array in generate_grid's layout, or a geometry —
    any tree create() evaluates, which is evaluated to a resident field on the grid first; `axes`: as for mesh.isosurface
    / mesh.contour; `band`: None, or the finite positive distance the result is cut at (and the search with it);
    `near`: "gradient" (step 4) or "seeds" (the distance to the seeds alone); `stats`: a dict that receives `seeds` and
    `ms`."""
    tables = _axes(axes)
    lv, bd, nr = _level(level), _band(band), _near(near)
    n = int(np.prod([t.size for t in tables]))
    geometry = _is_geometry(field)
    if not geometry and _points(field) != n:
        raise ValueError("the field has %d values; the axes span %s = %d points"
                         % (_points(field), "x".join(str(t.size) for t in tables), n))
    _engine.require_gpu()
    from ._eval import config
    own = None
    try:
        if geometry:
            own = dev = field.create_resident(_grid_of(axes)())
        elif isinstance(field, _engine.DeviceField):
            dev = field
            dev._live()
        else:
            own = dev = _engine.DeviceField.from_host(np.asarray(field, dtype=np.float32).ravel(), config.device)
        out = _engine.DeviceField(n, dev.device)
        try:
            field_redistance(dev.ptr, tables, lv, bd, nr, out.ptr, stats)
            if resident:
                return out
            return out.numpy()
        except BaseException:
            resident = False
            raise
        finally:
            if not resident:
                out.free()
    finally:
        if own is not None:
            own.free()


def from_geometry(geometry, size, resolution, level=0.0, band=None, near="gradient", resident=False):
    """redistance() of `geometry` on the grid generate_grid(size, resolution) spans (2 or 3 sizes)."""
    from .cores import generate_grid
    if len(size) not in (2, 3):
        raise ValueError("from_geometry: size has 2 or 3 entries")
    _level(level), _band(band), _near(near)
    if not _is_geometry(geometry):
        raise ValueError("from_geometry takes a geometry; redistance() takes fields")
    return redistance(geometry, generate_grid(size, resolution)[0], level, band, near, resident)
