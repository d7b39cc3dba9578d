"""Plane stacks of a geometry: the contours of its cross-sections on a stack of parallel planes, and their section
measures, on the GPU (kernels: csrc/sdfk_slices.inc).

    from aegolius_amd import slices
    s = slices.from_geometry(geometry, (2, 2, 2), (257, 257, 257))       # z-sections on generate_grid's tables
    s.layer(128).loops()                                                  # one layer as a mesh.Contour
    m = slices.measures(geometry, (U, V), heights, normal=slices.Frame((0, 0, 0.1), u, v))
    m.area, m.perimeter, m.volume()

Definition. A frame is an origin o and orthonormal u, v, n = u x v. A stack is a frame, in-plane tables U (nu >= 2) and
V (nv >= 2) and heights H (L >= 1), all strictly increasing as float32. Its field is F[l, i, j] = the geometry's value at
o + U[i] u + V[j] v + H[l] n. Layer l is the contour mesh.contour defines on the 2-D field F[l] with axes (U, V), bit
for bit: the inside rule f <= level, the vertex order (owner point, axis), the vertex arithmetic and the segments in
(cell, table) order with the inside on the left. The stack's vertices (V, 2) float32 as (a, b) and segments (S, 2) int64
are the layers' arrays one after the other, vertex ids global; `vertex_offsets` / `segment_offsets` (L + 1,) bound every
layer's range. No vertex sits between two layers and no cell spans two.

The field is the geometry seen through the frame (Frame.apply: one coordinate transform in front of the unchanged
program), evaluated on the native grid (H, U, V) — the layer is the slowest axis. For normal = 0 the frame is the
identity; normal = 1 and 2 are cyclic permutations, exact in float32, so that axis sections are sections of exactly what
create() evaluates.

Section measures of layer l, in float64 from the float32 vertices, relative to the centre (ca, cb) of the rectangle
[U[0], U[-1]] x [V[0], V[-1]]; for segment s from (a0, b0) to (a1, b1), t_s = (a0 - ca)(b1 - cb) - (a1 - ca)(b0 - cb):
area = sum t_s / 2, perimeter = sum hypot(a1 - a0, b1 - b0), first moments sum (a0 + a1 - 2 ca) t_s / 6 (and in b),
centroid = (ca, cb) + moments / area. A vertex with a == U[0], a == U[-1], b == V[0] or b == V[-1] is a border crossing:
the contour leaves the grid there, the layer is open, and its area and centroid are NaN (its perimeter is kept).

Not here: field input (only geometries), staged trees (grid-neighbourhood operators: refused), more than one GPU, and
toolpath infill (the layers are boundaries only).
"""
import numpy as np

from .cores.geom import GenericGeometry
from .mesh import Contour, _is_geometry, _level


class Frame:
    """Origin and orthonormal in-plane directions u, v of a plane stack; `normal` = u x v. Grid coordinates (h, a, b)
    are the world point origin + a u + b v + h normal."""

    def __init__(self, origin=(0.0, 0.0, 0.0), u=(1.0, 0.0, 0.0), v=(0.0, 1.0, 0.0)):
        vec = []
        for name, x in (("origin", origin), ("u", u), ("v", v)):
            x = np.asarray(x, dtype=np.float64)
            if x.shape != (3,) or not np.all(np.isfinite(x)):
                raise ValueError("Frame: %s must be 3 finite numbers" % name)
            vec.append(x.copy())
        self.origin, self.u, self.v = vec
        tol = 1e-12
        if abs(self.u.dot(self.u) - 1.0) > tol or abs(self.v.dot(self.v) - 1.0) > tol:
            raise ValueError("Frame: u and v must have unit length (|u|^2 = %.17g, |v|^2 = %.17g)"
                             % (self.u.dot(self.u), self.v.dot(self.v)))
        if abs(self.u.dot(self.v)) > tol:
            raise ValueError("Frame: u and v must be orthogonal (u . v = %.3g)" % self.u.dot(self.v))
        self.normal = np.cross(self.u, self.v)

    @classmethod
    def axis(cls, k):
        """The frame of sections normal to coordinate axis k (0, 1, 2) through the origin: u, v the two other axes in
        cyclic order, so that (normal, u, v) is (x, y, z), (y, z, x) or (z, x, y)."""
        if k not in (0, 1, 2):
            raise ValueError("Frame.axis: the normal is axis 0, 1 or 2; got %r" % (k,))
        e = np.eye(3)
        return cls((0.0, 0.0, 0.0), e[(k + 1) % 3], e[(k + 2) % 3])

    @property
    def matrix(self):
        """(3, 3) float64 with columns normal, u, v: world = origin + matrix . (h, a, b)."""
        return np.stack([self.normal, self.u, self.v], axis=1)

    def world(self, h, a, b):
        """World points (..., 3) float64 of grid coordinates (h, a, b) (broadcast against each other)."""
        h, a, b = np.broadcast_arrays(np.asarray(h, dtype=np.float64), np.asarray(a, dtype=np.float64),
                                      np.asarray(b, dtype=np.float64))
        return self.origin + h[..., None] * self.normal + a[..., None] * self.u + b[..., None] * self.v

    def apply(self, geometry):
        """A new geometry whose create(co) is `geometry` at the world points of co = (h, a, b); `geometry` is not
        changed. Lowered as one coordinate transform in front of the unchanged program of `geometry`, never merged
        into the geometry's own rotation."""
        if not _is_geometry(geometry):
            raise TypeError("Frame.apply: a geometry (GenericGeometry) is needed; got %r" % (type(geometry).__name__,))
        return FramedGeometry(self, geometry)

    def __repr__(self):
        return "Frame(origin=%r, u=%r, v=%r)" % (tuple(self.origin), tuple(self.u), tuple(self.v))


class FramedGeometry(GenericGeometry):
    """`inner` seen through a Frame (Frame.apply). To the lowering and the oracle it is a node with the rotation
    matrix^T and the centre -matrix^T origin, that is co' = matrix co + origin; the lowering takes `frame_map` instead,
    the matrix and offset as they are (no product of two roundings), while this node's own transform is the frame's."""

    def __init__(self, frame, inner):
        GenericGeometry.__init__(self, inner.propagate)
        self.frame, self.inner = frame, inner
        m = frame.matrix
        self._rot_matrix = m.T.copy()
        self._center = -(m.T.dot(frame.origin))
        self._framed = (self._rot_matrix.copy(), self._center.copy())

    @property
    def frame_map(self):
        """(A, c) of the transform q = A p - c the lowering emits; None once the node was moved, rotated or rescaled
        after the frame was applied (it is an ordinary node then)."""
        if (self._scale == 1 and np.array_equal(self._rot_matrix, self._framed[0])
                and np.array_equal(self._center, self._framed[1])):
            return self.frame.matrix, -self.frame.origin
        return None


class SectionMeasures:
    """Per-layer measures of a plane stack: `area` (L,), `perimeter` (L,), `centroid` (L, 2) as (a, b), `moments` (L, 2)
    (the first moments about the rectangle's centre), `segments` (L,) int64, `border` (L,) int64 border crossings,
    `closed` (L,) bool, `heights` (L,). Area and centroid of an open layer are NaN."""

    def __init__(self, raw, heights, centre):
        raw = np.asarray(raw, dtype=np.float64).reshape(-1, 6)
        self.heights = np.asarray(heights, dtype=np.float64)
        self.segments = raw[:, 4].astype(np.int64)
        self.border = raw[:, 5].astype(np.int64)
        self.closed = self.border == 0
        self.perimeter = raw[:, 1].copy()
        self.area = np.where(self.closed, raw[:, 0], np.nan)
        self.moments = raw[:, 2:4].copy()
        with np.errstate(divide="ignore", invalid="ignore"):
            self.centroid = np.asarray(centre, dtype=np.float64) + raw[:, 2:4] / self.area[:, None]

    def __len__(self):
        return len(self.heights)

    def volume(self):
        """Trapezoid rule of `area` over `heights` (0 for a single layer); NaN if any layer is open."""
        if not np.all(self.closed):
            return float("nan")
        return float(np.sum(0.5 * (self.area[1:] + self.area[:-1]) * np.diff(self.heights)))


def _centre(axes):
    return (0.5 * (float(axes[0][0]) + float(axes[0][-1])), 0.5 * (float(axes[1][0]) + float(axes[1][-1])))


def section_sums(vertices, segments, vertex_offsets, segment_offsets, axes):
    """The (L, 6) sums of the definition from a stack's arrays, numpy float64, segments added in their order: area,
    perimeter, first moments in a and b, segments, border crossings."""
    v = np.asarray(vertices, dtype=np.float32)
    seg = np.asarray(segments, dtype=np.int64)
    ca, cb = _centre(axes)
    u0, u1, v0, v1 = axes[0][0], axes[0][-1], axes[1][0], axes[1][-1]
    out = np.zeros((len(vertex_offsets) - 1, 6), dtype=np.float64)
    for l in range(len(out)):
        s = seg[segment_offsets[l]:segment_offsets[l + 1]]
        p0, p1 = v[s[:, 0]].astype(np.float64), v[s[:, 1]].astype(np.float64)
        a0, b0, a1, b1 = p0[:, 0] - ca, p0[:, 1] - cb, p1[:, 0] - ca, p1[:, 1] - cb
        t = a0 * b1 - a1 * b0
        mine = v[vertex_offsets[l]:vertex_offsets[l + 1]]
        on = (mine[:, 0] == u0) | (mine[:, 0] == u1) | (mine[:, 1] == v0) | (mine[:, 1] == v1)
        out[l] = (0.5 * t.sum(), np.hypot(p1[:, 0] - p0[:, 0], p1[:, 1] - p0[:, 1]).sum(), ((a0 + a1) * t / 6.0).sum(),
                  ((b0 + b1) * t / 6.0).sum(), len(s), np.count_nonzero(on))
    return out


class SliceStack:
    """A plane stack: `vertices` (V, 2) float32 as (a, b), `segments` (S, 2) int64 with global vertex ids and the inside
    on the left, `vertex_offsets` / `segment_offsets` (L + 1,) int64, `heights` (L,) float32, `frame`, `axes` = (U, V)
    float32."""

    def __init__(self, vertices, segments, vertex_offsets, segment_offsets, heights, frame, axes):
        self.vertices, self.segments = vertices, segments
        self.vertex_offsets, self.segment_offsets = vertex_offsets, segment_offsets
        self.heights, self.frame, self.axes = heights, frame, tuple(axes)

    def __len__(self):
        return len(self.heights)

    def __repr__(self):
        return "SliceStack(%d layers, %d vertices, %d segments)" % (len(self), len(self.vertices), len(self.segments))

    def layer(self, l):
        """Layer l as a mesh.Contour of its own: its vertices, its segments with ids counted from its first vertex
        (loops() chains them; project() takes a geometry of the (a, b) plane — the Newton step of a 3-D geometry would
        leave the layer)."""
        l = range(len(self))[l]
        v0, v1 = int(self.vertex_offsets[l]), int(self.vertex_offsets[l + 1])
        s0, s1 = int(self.segment_offsets[l]), int(self.segment_offsets[l + 1])
        return Contour(self.vertices[v0:v1].copy(), np.asarray(self.segments[s0:s1], dtype=np.int64) - v0)

    def world_vertices(self):
        """(V, 3) float64: every vertex in world coordinates, frame.world(height of its layer, a, b)."""
        h = np.repeat(np.asarray(self.heights, dtype=np.float64), np.diff(self.vertex_offsets))
        v = np.asarray(self.vertices, dtype=np.float64).reshape(-1, 2)
        return self.frame.world(h, v[:, 0], v[:, 1]).reshape(-1, 3)

    def measures(self):
        """The SectionMeasures of the downloaded arrays, in numpy float64 (what `measures` computes on the device, up to
        the order of the sums)."""
        raw = section_sums(self.vertices, self.segments, self.vertex_offsets, self.segment_offsets, self.axes)
        return SectionMeasures(raw, self.heights, _centre(self.axes))

    def write_svg(self, path, layer):
        """Layer `layer` as an SVG file: one <path> per loop of its contour (closed loops end in Z), in the (a, b)
        plane with b pointing up."""
        c = self.layer(layer)
        u, v = self.axes
        w, h = float(u[-1]) - float(u[0]), float(v[-1]) - float(v[0])
        lines = ['<svg xmlns="http://www.w3.org/2000/svg" viewBox="%.9g %.9g %.9g %.9g">' % (float(u[0]), -float(v[-1]), w, h),
                 '<g transform="scale(1,-1)" fill="none" stroke="black" stroke-width="%.9g">' % (0.002 * max(w, h))]
        for loop in c.loops():
            closed = len(loop) > 1 and loop[0] == loop[-1]
            pts = c.vertices[loop[:-1] if closed else loop]
            d = "M " + " L ".join("%.9g,%.9g" % (float(a), float(b)) for a, b in pts) + (" Z" if closed else "")
            lines.append('<path d="%s"/>' % d)
        lines += ["</g>", "</svg>"]
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def _table(values, name, least):
    t = np.ascontiguousarray(np.asarray(values, dtype=np.float64).ravel(), dtype=np.float32)
    if t.size < least:
        raise ValueError("%s has %d point(s); it needs at least %d" % (name, t.size, least))
    if not np.all(np.isfinite(t)) or not np.all(t[1:] > t[:-1]):
        raise ValueError("%s is not strictly increasing (as float32)" % name)
    return t


def _frame(normal):
    if isinstance(normal, Frame):
        return normal
    if isinstance(normal, (int, np.integer)) and not isinstance(normal, bool) and int(normal) in (0, 1, 2):
        return Frame.axis(int(normal))
    raise ValueError("normal: 0, 1, 2 or a Frame; got %r" % (normal,))


def _prepare(geometry, axes, heights, normal, level):
    """-> (program of the framed geometry, tables (H, U, V), level, frame); every check before any device work."""
    from ._eval import program_for
    from ._lower import NeedsStage, lower_geometry
    if not _is_geometry(geometry):
        raise TypeError("slices: a geometry (GenericGeometry) is needed — fields are not sliced; got %r"
                        % (type(geometry).__name__,))
    frame = _frame(normal)
    lv = _level(level)
    if len(axes) != 2:
        raise ValueError("axes: the two in-plane tables (U, V); got %d" % len(axes))
    tables = [_table(heights, "heights", 1), _table(axes[0], "axis U", 2), _table(axes[1], "axis V", 2)]
    try:
        lowered = lower_geometry(frame.apply(geometry))
    except NeedsStage as need:
        raise ValueError("slices: the tree holds the grid operator %r, which is evaluated on the grid it was made for "
                         "(a staged tree); it has no meaning on the layer grid of a plane stack" % (need.expr.name,)) from None
    return program_for(lowered), tables, lv, frame


# ---- public interface -------------------------------------------------------------------------------------------------------
def stack(geometry, axes, heights, normal=2, level=0.0, timings=None):
    """The plane stack of {geometry = level}: `axes` = (U, V) in-plane tables, `heights` along the normal, `normal` the
    coordinate axis 0, 1, 2 (Frame.axis) or a Frame. `timings`: a dict that receives device-event milliseconds of count
    (evaluation to inside bits, count, scans, layer offsets) / emit / copy. -> SliceStack."""
    from ._eval import config
    prog, tables, lv, frame = _prepare(geometry, axes, heights, normal, level)
    verts, segs, voff, soff = prog.slices_grid(tables, lv, device=config.device, mode=config.mode, timings=timings)
    return SliceStack(verts, segs.astype(np.int64, copy=False), voff, soff, tables[0], frame, tables[1:])


def measures(geometry, axes, heights, normal=2, level=0.0, timings=None):
    """The SectionMeasures of the same stack, reduced per layer on the device: no contour crosses PCIe, 6 doubles per
    layer come back. `timings`: a dict that receives the device-event milliseconds of the call (measure)."""
    from ._eval import config
    prog, tables, lv, _ = _prepare(geometry, axes, heights, normal, level)
    raw, _, _ = prog.slices_measure_grid(tables, lv, device=config.device, mode=config.mode, timings=timings)
    return SectionMeasures(raw, tables[0], _centre(tables[1:]))


def from_geometry(geometry, size, resolution, normal=2, level=0.0):
    """stack() on the grid generate_grid(size, resolution) spans (3 sizes), from its axis tables: for normal k the
    table of axis k becomes the heights and the two others (U, V) in cyclic order; for a Frame the three tables are
    (heights, U, V) as they come."""
    from .cores.helper_functions import grid_axes
    if len(size) != 3:
        raise ValueError("from_geometry: size has 3 entries")
    axes, _ = grid_axes(size, resolution)
    frame = _frame(normal)
    k = 0 if frame is normal else int(normal)
    return stack(geometry, (axes[(k + 1) % 3], axes[(k + 2) % 3]), axes[k], normal, level)
