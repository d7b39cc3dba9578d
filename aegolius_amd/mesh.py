"""Isosurface meshes and 2-D contours of scalar fields, extracted on the GPU (kernels: csrc/sdfk_mesh.inc).

    from aegolius_amd import mesh
    m = mesh.from_geometry(geometry, (2, 2, 2), (257, 257, 257))      # or mesh.isosurface(geometry or device_field, co)
    m.compute_normals(geometry)
    m.write_ply("part.ply")

The field stays in HBM (a DeviceField, or a host array uploaded once); only the mesh crosses PCIe. A geometry is meshed
without a field at all: its evaluation writes one inside bit per grid point, and it is evaluated again only at the two
ends of every crossing edge ("geometry path") — the same output, bit for bit, as meshing its field.

Output definition (the kernels and tests/mesh_reference.py implement exactly this):
  * A grid point is inside if f <= level. NaN is outside.
  * Point (i, j, k) owns its grid edges in +x, +y and +z. There is one vertex per edge whose two ends differ in the inside
    test, ordered by the owning point's linear index (C order, z fastest), then by axis. Along the edge's axis the vertex
    sits at x = xa + t * (xb - xa), t = (level - fa) / (fb - fa), in float32 and this operation order, a the lower end;
    the other coordinates are the axis values. If one end is NaN, the vertex is put at the other end.
  * Triangles are ordered by cell (the index of its minimum corner in the (nx-1)(ny-1)(nz-1) cells, C order), then by
    the order of the generated case table (aegolius_amd/_mctable.py: one face rule, diagonal inside corners separated,
    so that the mesh is watertight). (v1 - v0) x (v2 - v0) points toward increasing f.
  * 2-D: the same per square (16 cases); point (i, j) owns its +x and +y edges; each segment (a, b) has the inside on
    its left, so an inside region is bounded counter-clockwise and a hole clockwise.
"""
import contextlib
import struct

import numpy as np

from . import _engine


class Mesh:
    """A triangle mesh: vertices (V, 3) float32, faces (F, 3) int64, normals None or (V, 3) float32."""

    def __init__(self, vertices, faces, normals=None):
        self.vertices = vertices
        self.faces = faces
        self.normals = normals

    def __repr__(self):
        return "Mesh(%d vertices, %d faces)" % (len(self.vertices), len(self.faces))

    def compute_normals(self, geometry):
        """Unit gradient of `geometry` at every vertex (autodiff.value_and_grad_points, normalised on the host).
        Raises that function's UnsupportedOpError for trees without a dual rule."""
        from .autodiff import value_and_grad_points
        _, grad = value_and_grad_points(geometry, np.ascontiguousarray(self.vertices.T, dtype=np.float32))
        g = np.asarray(grad, dtype=np.float64).reshape(3, -1).T
        norm = np.linalg.norm(g, axis=1, keepdims=True)
        self.normals = np.ascontiguousarray(np.divide(g, norm, out=np.zeros_like(g), where=norm > 0), dtype=np.float32)
        return self.normals

    def project(self, geometry, level=0.0, **kw):
        """Move the vertices onto {geometry = level} in place (surface.project from every vertex; `kw`: its tol,
        max_iter, relax) and set `normals` from the gradients at the projected points. `faces` stays as it is; a vertex
        whose status is not CONVERGED stays where it was. -> the SurfacePoints of the vertices."""
        from .surface import _project_vertices
        sp, self.vertices, self.normals = _project_vertices(self.vertices, geometry, level, kw, 3)
        return sp

    def write_obj(self, path):
        v = np.asarray(self.vertices, dtype=np.float32)
        with open(path, "w") as f:
            f.write("# %d vertices, %d faces\n" % (len(v), len(self.faces)))
            if len(v):
                np.savetxt(f, v, fmt="v %.9g %.9g %.9g")
            if self.normals is not None and len(v):
                np.savetxt(f, np.asarray(self.normals, dtype=np.float32), fmt="vn %.9g %.9g %.9g")
            if len(self.faces):
                fi = np.asarray(self.faces, dtype=np.int64) + 1
                if self.normals is not None:
                    np.savetxt(f, np.repeat(fi, 2, axis=1), fmt="f %d//%d %d//%d %d//%d")
                else:
                    np.savetxt(f, fi, fmt="f %d %d %d")

    def write_ply(self, path):
        """Binary little-endian PLY: float x y z (and nx ny nz), faces as uchar-counted int lists."""
        v = np.asarray(self.vertices, dtype="<f4")
        if len(v) > 0x7fffffff:
            raise ValueError("PLY int vertex indices hold fewer than 2^31 vertices")
        props = ["x", "y", "z"] + (["nx", "ny", "nz"] if self.normals is not None else [])
        head = ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(v)]
        head += ["property float %s" % p for p in props]
        head += ["element face %d" % len(self.faces), "property list uchar int vertex_indices", "end_header"]
        vrec = np.empty(len(v), dtype=[(p, "<f4") for p in props])
        for i, p in enumerate("xyz"):
            vrec[p] = v[:, i]
        if self.normals is not None:
            nrm = np.asarray(self.normals, dtype="<f4")
            for i, p in enumerate(("nx", "ny", "nz")):
                vrec[p] = nrm[:, i]
        frec = np.empty(len(self.faces), dtype=[("n", "u1"), ("i", "<i4", (3,))])
        frec["n"] = 3
        frec["i"] = np.asarray(self.faces)
        with open(path, "wb") as f:
            f.write(("\n".join(head) + "\n").encode("ascii"))
            f.write(vrec.tobytes())
            f.write(frec.tobytes())

    def write_stl(self, path):
        """Binary STL. Facet normals: the normalised mean of the vertex normals when present, else of the face's
        (v1 - v0) x (v2 - v0)."""
        v = np.asarray(self.vertices, dtype=np.float32)
        tri = v[np.asarray(self.faces, dtype=np.int64)].astype(np.float64) if len(self.faces) else np.zeros((0, 3, 3))
        if self.normals is not None and len(self.faces):
            nrm = np.asarray(self.normals, dtype=np.float64)[np.asarray(self.faces)].sum(axis=1)
        else:
            nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        length = np.linalg.norm(nrm, axis=1, keepdims=True)
        nrm = np.divide(nrm, length, out=np.zeros_like(nrm), where=length > 0)
        rec = np.zeros(len(tri), dtype=[("n", "<f4", (3,)), ("v", "<f4", (3, 3)), ("attr", "<u2")])
        rec["n"] = nrm
        rec["v"] = v[np.asarray(self.faces, dtype=np.int64)] if len(self.faces) else np.zeros((0, 3, 3))
        with open(path, "wb") as f:
            f.write(b"aegolius_amd isosurface".ljust(80, b" "))
            f.write(struct.pack("<I", len(rec)))
            f.write(rec.tobytes())


class Contour:
    """Contour segments: vertices (V, 2) float32, segments (S, 2) int64 with the inside on the left of a -> b;
    normals None, or (V, 3) float32 after project()."""

    def __init__(self, vertices, segments):
        self.vertices = vertices
        self.segments = segments
        self.normals = None

    def __repr__(self):
        return "Contour(%d vertices, %d segments)" % (len(self.vertices), len(self.segments))

    def project(self, geometry, level=0.0, **kw):
        """Mesh.project for a contour: the vertices move in the plane (z is 0 and stays 0: every 2-D rule's z tangent is
        exactly 0), `normals` (V, 3) float32 is set, `segments` stays as it is. -> the SurfacePoints of the vertices."""
        from .surface import _project_vertices
        sp, self.vertices, self.normals = _project_vertices(self.vertices, geometry, level, kw, 2)
        return sp

    def loops(self):
        """The segments chained into polylines of vertex ids: closed loops first (their first vertex repeated at the
        end), then open chains (they end on the grid's border), each group in the order of its first segment. Closed
        loops run counter-clockwise around inside regions and clockwise around holes."""
        seg = np.asarray(self.segments, dtype=np.int64)
        nxt = {}
        has_in = set()
        for s, (a, b) in enumerate(seg.tolist()):
            nxt[a] = (b, s)
            has_in.add(b)
        used = np.zeros(len(seg), dtype=bool)
        closed, open_ = [], []
        for s, (a, _) in enumerate(seg.tolist()):       # open chains start at a vertex nothing leads to
            if a in has_in or used[s]:
                continue
            chain, v = [a], a
            while v in nxt and not used[nxt[v][1]]:
                v, k = nxt[v]
                used[k] = True
                chain.append(v)
            open_.append((s, np.asarray(chain, dtype=np.int64)))
        for s, (a, _) in enumerate(seg.tolist()):
            if used[s]:
                continue
            chain, v = [a], a
            while not used[nxt[v][1]]:
                v, k = nxt[v]
                used[k] = True
                chain.append(v)
            closed.append(np.asarray(chain, dtype=np.int64))
        return closed + [c for _, c in sorted(open_, key=lambda x: x[0])]


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def _tables(axes, dims):
    """axes: a sequence of 1-D arrays, or a generate_grid array with its grid_axes tag -> list of float32 tables."""
    tagged = getattr(axes, "grid_axes", None)
    if tagged is not None:
        axes = tagged
    elif isinstance(axes, np.ndarray) and axes.ndim == 2 and axes.shape[0] == 3:
        raise ValueError("axes: a generate_grid array that is no longer tagged with its axis tables (it was written to or "
                         "copied); pass the three axis arrays instead")
    tables = [np.ascontiguousarray(np.asarray(a, dtype=np.float64).ravel(), dtype=np.float32) for a in axes]
    if dims == 2 and len(tables) == 3:
        if tables[2].size != 1 or tables[2][0] != 0.0:
            raise ValueError("contour: three axes are accepted only from a 2-D grid, whose third axis is the single 0.0")
        tables = tables[:2]
    if len(tables) != dims:
        raise ValueError("expected %d axis tables, got %d" % (dims, len(tables)))
    for a, t in enumerate(tables):
        if t.size < 2:
            raise ValueError("axis %d has %d point(s); every axis needs at least 2" % (a, t.size))
        if not np.all(t[1:] > t[:-1]):
            raise ValueError("axis %d is not strictly increasing (as float32)" % a)
    return tables


def _level(level):
    lv = np.float32(level)
    if np.isnan(lv):
        raise ValueError("the level is NaN")
    return float(lv)


def _points(field):
    if isinstance(field, _engine.DeviceField):
        return field.n
    return int(np.asarray(field).size)


def _extract(field, tables, level, timings=None):
    dims = len(tables)
    shape = tuple(t.size for t in tables)
    n = int(np.prod(shape))
    if _points(field) != n:
        raise ValueError("the field has %d values; the axes span %s = %d points" % (_points(field), "x".join(map(str, shape)), n))
    lv = _level(level)
    with contextlib.ExitStack() as stack:
        if isinstance(field, _engine.DeviceField):
            dev = field
            dev._live()
        else:
            dev = stack.enter_context(_engine.DeviceField.from_host(np.asarray(field, dtype=np.float32).ravel(), _device()))
        _, tab = _engine.axis_args(tables)
        d_field = (_engine._vp(dev.ptr),)
        verts, faces = _engine.extract_mesh("sdfk_field", shape, lv, d_field + tab, d_field + shape, timings=timings)
    return verts, faces.astype(np.int64, copy=False)


def _device():
    from ._eval import config
    return config.device


# ---- geometries -------------------------------------------------------------------------------------------------------------
def _is_geometry(obj):
    from .cores.geom import GenericGeometry
    return isinstance(obj, GenericGeometry)


def _grid_array(axes):
    """The tagged (3, N) grid of the axis tables (what generate_grid returns), for trees evaluated to a field first."""
    from .cores.helper_functions import GridCoords
    ax = [np.asarray(a, dtype=np.float64).ravel() for a in axes]
    ax += [np.zeros(1)] * (3 - len(ax))
    n = [a.size for a in ax]
    co = GridCoords((3, n[0] * n[1] * n[2]), dtype=np.float64)
    shaped = np.asarray(co).reshape(3, *n)
    shaped[0] = ax[0][:, None, None]
    shaped[1] = ax[1][None, :, None]
    shaped[2] = ax[2][None, None, :]
    co._grid_axes = ax
    co.setflags(write=False)
    return co


def _extract_geometry(geometry, tables, level, timings, grid):
    """Mesh of a geometry on the grid of `tables`. A tree that lowers to one program is evaluated to inside bits and at
    the crossing edges' ends only (_engine.Program.mesh_grid); a staged tree (NeedsStage) is evaluated to a resident
    field on the grid `grid()` returns, which is then meshed — the rule of _eval.select_geometry."""
    from ._eval import config, program_for
    from ._lower import NeedsStage, lower_geometry
    lv = _level(level)
    geometry._sdf = geometry.modified_object                   # (as create() does)
    try:
        lowered = lower_geometry(geometry)
    except NeedsStage:
        dev = geometry.create_resident(grid())
        try:
            return _extract(dev, tables, lv, timings)
        finally:
            dev.free()
    verts, faces = program_for(lowered).mesh_grid(tables, lv, device=config.device, mode=config.mode, timings=timings)
    return verts, faces.astype(np.int64, copy=False)


def _grid_of(axes):
    return lambda: axes if getattr(axes, "grid_axes", None) is not None else _grid_array(axes)


# ---- public interface -------------------------------------------------------------------------------------------------------
def isosurface(field, axes, level=0.0, timings=None):
    """Triangle mesh of {f = level} of a 3-D field. `field`: a DeviceField, a host array of nx ny nz values in C order
    (generate_grid's layout), or a geometry (GenericGeometry: any tree create() evaluates), meshed without a field or a
    coordinate array; `axes`: three strictly increasing 1-D arrays (lengths nx, ny, nz, each >= 2, uniform or not) or a
    generate_grid array. `timings`: a dict that receives device-event milliseconds of count / emit / copy (a geometry's
    evaluation to inside bits is part of count)."""
    tables = _tables(axes, 3)
    if _is_geometry(field):
        verts, faces = _extract_geometry(field, tables, level, timings, _grid_of(axes))
    else:
        verts, faces = _extract(field, tables, level, timings)
    return Mesh(verts, faces)


def contour(field, axes, level=0.0, timings=None):
    """Segments of {f = level} of a 2-D field of nx ny values, or of a geometry on that grid: `axes` is (x, y), or the
    three axes / the array of a 2-D generate_grid (third axis the single 0.0). The shape is taken from the axes."""
    tables = _tables(axes, 2)
    if _is_geometry(field):
        verts, segs = _extract_geometry(field, tables, level, timings, _grid_of(axes))
    else:
        verts, segs = _extract(field, tables, level, timings)
    return Contour(verts, segs)


def from_geometry(geometry, size, resolution, level=0.0):
    """isosurface (3 sizes) or contour (2 sizes) of `geometry` on the grid generate_grid(size, resolution) spans, from
    its axis tables (grid_axes): neither the coordinate array nor a field is made, except for staged trees, which are
    evaluated to a field on generate_grid's array first."""
    from .cores.helper_functions import grid_axes
    dims = len(size)
    if dims not in (2, 3):
        raise ValueError("from_geometry: size has 2 (contour) or 3 (isosurface) entries")
    axes, _ = grid_axes(size, resolution)
    tables = _tables(axes, dims)

    def grid():
        from .cores import generate_grid
        return generate_grid(size, resolution)[0]
    verts, faces = _extract_geometry(geometry, tables, level, None, grid)
    return Mesh(verts, faces) if dims == 3 else Contour(verts, faces)
