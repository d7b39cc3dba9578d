"""Topology of a solid on a grid, on the GPU: connected components with their sizes and boxes, enclosed cavities and
through-holes (kernels: csrc/sdfk_topology.inc).

    from aegolius_amd import topology, redistance
    c = topology.from_geometry(geometry, (2, 2, 2), (257, 257, 257))     # or topology.label(field or geometry, axes)
    c.count, c.sizes, c.box(c.largest())                                 # islands, their points, the body's box
    body = c.field(keep=[c.largest()])                                   # a DeviceField: the body without its debris
    d = redistance.redistance(body, axes)
    t = topology.betti(geometry, axes)                                   # t.components, t.tunnels, t.cavities, t.euler

Definitions (the kernels and tests/topology_reference.py implement exactly this):
  * Grid. D = 2 or 3 strictly increasing axis tables of at least 2 points each; points in C order, the linear index p as
    in `mesh`. At most 2^31 - 1 points, because labels are int32 (1290^3 is the practical limit).
  * Inside. A point is inside iff f <= level by the mesh's rule (the comparison of selection keys); NaN counts as outside.
  * region. "inside" labels the inside points, "outside" all the others.
  * connectivity. "faces": 4 neighbours in 2-D, 6 in 3-D. "full": 8 and 26.
  * Canonical name. A component's name is the smallest linear index among its points (`first`); components are numbered
    0 .. K - 1 by ascending `first`. Every output is therefore independent of scheduling: two runs, or the GPU and the
    reference, agree exactly, not up to relabelling.
  * Record, per component: `first` (int64), `size` in points (int64), the index bounding box `lower[D]`, `upper[D]`
    (int32, both ends included) and `border`, true when any of its points lies on a face of the grid.
  * Cell counts. V = inside points, E = grid edges with both ends inside, F = grid squares with all 4 corners inside,
    C = grid cubes with all 8 corners inside (3-D only), all int64; euler = V - E + F - C (2-D: V - E + F).
  * Betti numbers of the cubical complex the inside points span (a cell belongs to it iff all its corners are inside):
    b0 = components of the inside under "faces"; 3-D: b2 = components of the outside under "full" that do not touch the
    border, b1 = b0 + b2 - euler; 2-D: b1 = b0 - euler, which must equal the number of outside "full" components that
    do not touch the border — `betti` computes both and raises if they disagree.

A geometry whose tree lowers to one program is evaluated to one inside bit per point: no field and no coordinate array
exist. A staged tree (grid operators such as conv_averaging) is evaluated to a resident field first, as in `mesh`.

Not here: more than 2^31 - 1 points; more than one GPU; periodic grids; per-component mass properties (the route for now
is `field(keep=[k])` into `moments`); the layers of a plane stack labelled as separate 2-D problems.
"""
import numpy as np

from . import _engine
from .mesh import _grid_of, _is_geometry, _level, _points, _tables

CONNECTIVITY = ("faces", "full")
REGION = ("inside", "outside")
MAX_POINTS = 2 ** 31 - 1


class Components:
    """The components of one labelling: `count` K, `first` (K,) int64, `sizes` (K,) int64, `lower` / `upper` (K, D) int32,
    `border` (K,) bool as host arrays; `shape`, `connectivity`, `region`, `level`, `axes` (the float32 tables);
    `labels`: the device-resident int32 ids (an _engine.DeviceBuffer of prod(shape) entries, -1 off the region), None
    after label(..., labels=False) or free(). The buffer is freed with the object."""

    def __init__(self, records, labels, tables, connectivity, region, level, device):
        self.first, self.sizes, self.lower, self.upper, self.border = records
        self.count = int(len(self.first))
        self.labels = labels
        self.axes = tuple(tables)
        self.shape = tuple(int(t.size) for t in tables)
        self.connectivity, self.region, self.level, self.device = connectivity, region, level, device

    def __len__(self):
        return self.count

    def __repr__(self):
        return "Components(%d %s components, %s, grid %s)" % (self.count, self.region, self.connectivity,
                                                              "x".join(map(str, self.shape)))

    def _labels(self):
        if self.labels is None or not self.labels.ptr:
            raise ValueError("the label array was dropped (labels=False) or freed")
        return self.labels

    def free(self):
        if self.labels is not None:
            self.labels.free()
        self.labels = None

    def labels_host(self):
        """The ids as a host array of `shape`, int32, -1 where the point is not in the region."""
        return self._labels().download(np.empty(self.shape, dtype=np.int32))

    def largest(self):
        """The id of the component with the most points; a tie goes to the lower id."""
        if self.count == 0:
            raise ValueError("there is no component")
        return int(np.argmax(self.sizes))

    def box(self, k):
        """World-coordinate bounding box of component k from the tables -> (lower (D,), upper (D,)) float64."""
        k = range(self.count)[k]
        lo = [float(t[i]) for t, i in zip(self.axes, self.lower[k])]
        hi = [float(t[i]) for t, i in zip(self.axes, self.upper[k])]
        return np.asarray(lo), np.asarray(hi)

    def field(self, keep=None, inside=-1.0, outside=1.0):
        """A DeviceField with `inside` at the points of the kept components and `outside` elsewhere, written by one
        kernel from the labels. `keep`: every id (default), a sequence of ids, or a boolean array of length K."""
        mask = np.ones(self.count, dtype=bool)
        if keep is not None:
            k = np.asarray(keep)
            if k.dtype == bool:
                if k.shape != (self.count,):
                    raise ValueError("keep: a boolean array has one entry per component (%d); got shape %r" % (self.count, k.shape))
                mask = k.copy()
            else:
                ids = np.asarray(keep, dtype=np.int64).ravel()
                if ids.size and (ids.min() < 0 or ids.max() >= self.count):
                    raise ValueError("keep: ids are 0 .. %d" % (self.count - 1))
                mask = np.zeros(self.count, dtype=bool)
                mask[ids] = True
        labels = self._labels()
        return _engine.label_field(labels, int(np.prod(self.shape)), mask, np.float32(inside), np.float32(outside), self.device)


class Topology:
    """Betti numbers of the cubical complex of the inside points: `components` (b0), `tunnels` (b1), `cavities` (b2; 0 in
    2-D, where `tunnels` counts the holes), `euler`, and the cell counts `vertices`, `edges`, `faces`, `cubes`; `shape`."""

    def __init__(self, components, tunnels, cavities, cells, shape):
        self.components, self.tunnels, self.cavities = int(components), int(tunnels), int(cavities)
        self.vertices, self.edges, self.faces, self.cubes = (int(c) for c in cells)
        self.euler = self.vertices - self.edges + self.faces - self.cubes
        self.shape = tuple(shape)

    def __repr__(self):
        return "Topology(components=%d, tunnels=%d, cavities=%d, euler=%d)" % (self.components, self.tunnels, self.cavities,
                                                                               self.euler)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def _axes(axes):
    """-> float32 tables (2 or 3) by mesh's rules: tables, the three of a 2-D grid, or a tagged generate_grid array."""
    tagged = getattr(axes, "grid_axes", None)
    given = tagged if tagged is not None else axes
    if tagged is None and isinstance(axes, np.ndarray) and axes.ndim == 2 and axes.shape[0] == 3:
        _tables(axes, 3)                                       # (raises: an untagged generate_grid array)
    given = [np.asarray(a).ravel() for a in given]
    if len(given) not in (2, 3):
        raise ValueError("topology: a grid has 2 or 3 axis tables; got %d" % len(given))
    flat = len(given) == 2 or (given[2].size == 1 and given[2][0] == 0.0)
    tables = _tables(axes, 2 if flat else 3)
    n = int(np.prod([t.size for t in tables], dtype=np.int64))
    if n > MAX_POINTS:
        raise ValueError("the axes span %s = %d points; labels are int32: at most 2^31 - 1 points"
                         % ("x".join(str(t.size) for t in tables), n))
    return tables


def _choice(value, names, what):
    if value not in names:
        raise ValueError("%s is one of %r; got %r" % (what, names, value))
    return names.index(value)


class _Session:
    """The scratch of one call and its source (`grid()`: the tagged coordinate array, made for a staged tree only): a program (one inside bit per point, no field), or a resident field — the
    caller's, an uploaded host array, or a staged tree evaluated by create_resident (the rule of mesh._extract_geometry)."""

    def __init__(self, source, grid, tables, level):
        from ._eval import config, program_for
        from ._lower import NeedsStage, lower_geometry
        self.level, self.mode, self.own, self.scratch = level, config.mode, None, None
        n = int(np.prod([t.size for t in tables], dtype=np.int64))
        geometry = _is_geometry(source)
        if not geometry and _points(source) != n:
            raise ValueError("the field has %d values; the axes span %s = %d points"
                             % (_points(source), "x".join(str(t.size) for t in tables), n))
        _engine.require_gpu()
        try:
            if geometry:
                source._sdf = source.modified_object           # (as create() does)
                try:
                    self.source = program_for(lower_geometry(source))
                except NeedsStage:
                    self.source = self.own = source.create_resident(grid())
            elif isinstance(source, _engine.DeviceField):
                source._live()
                self.source = source
            else:
                self.source = self.own = _engine.DeviceField.from_host(np.asarray(source, dtype=np.float32).ravel(), config.device)
            device = config.device if isinstance(self.source, _engine.Program) else self.source.device
            self.scratch = _engine.LabelScratch(tables, device)
        except BaseException:
            self.close()
            raise

    def close(self):
        for buf in (self.scratch, self.own):
            if buf is not None:
                buf.free()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---- public interface -------------------------------------------------------------------------------------------------------
def label(source, axes, level=0.0, connectivity="faces", region="inside", labels=True, timings=None):
    """The connected components of the region of {source <= level} on the grid of `axes` -> Components.
    `source`: a host array of prod(shape) values in C order, a DeviceField, or a geometry (any tree create() evaluates);
    `axes`: as for mesh.isosurface / mesh.contour (2 or 3 tables, or a generate_grid array); `labels=False` drops the
    device label array once the records are made. At most 2^31 - 1 points (labels are int32). `timings`: a dict that
    receives device-event milliseconds of bits / init / merge / compress / number."""
    return _label(source, _axes(axes), _grid_of(axes), level, connectivity, region, labels, timings)


def _label(source, tables, grid, level, connectivity, region, labels, timings):
    lv = _level(level)
    conn, reg = _choice(connectivity, CONNECTIVITY, "connectivity"), _choice(region, REGION, "region")
    with _Session(source, grid, tables, lv) as s:
        buf = s.scratch.labels()
        try:
            count = s.scratch.label(s.source, lv, conn, reg, buf, s.mode, timings)
            records = s.scratch.records(count, buf)
        except BaseException:
            buf.free()
            raise
        if not labels:
            buf.free()
            buf = None
        return Components(records, buf, tables, connectivity, region, lv, s.scratch.device)


def from_geometry(geometry, size, resolution, level=0.0, connectivity="faces", region="inside", labels=True):
    """label() of `geometry` on the grid generate_grid(size, resolution) spans (2 or 3 sizes), from its axis tables:
    neither the coordinate array nor a field is made, except for staged trees, which are evaluated to a field on
    generate_grid's array first."""
    from .cores.helper_functions import grid_axes
    if len(size) not in (2, 3):
        raise ValueError("from_geometry: size has 2 or 3 entries")
    if not _is_geometry(geometry):
        raise ValueError("from_geometry takes a geometry; label() takes fields")
    axes, _ = grid_axes(size, resolution)

    def grid():
        from .cores import generate_grid
        return generate_grid(size, resolution)[0]
    return _label(geometry, _axes(axes), grid, level, connectivity, region, labels, None)


def cell_counts(source, axes, level=0.0):
    """(V, E, F, C) of the cubical complex the inside points of {source <= level} span, as Python ints (C = 0 in 2-D)."""
    tables = _axes(axes)
    lv = _level(level)
    with _Session(source, _grid_of(axes), tables, lv) as s:
        return s.scratch.cell_counts(s.source, lv, s.mode)


def betti(source, axes, level=0.0):
    """Components, tunnels and cavities of {source <= level} on the grid of `axes` -> Topology. One bit string, two
    labellings of it (inside / faces, and outside / full on its complement) and one cell-count kernel; no label array
    outlives the call. Raises RuntimeError when, in 2-D, the holes by labelling and b0 - euler disagree."""
    tables = _axes(axes)
    lv = _level(level)
    with _Session(source, _grid_of(axes), tables, lv) as s:
        cells = s.scratch.cell_counts(s.source, lv, s.mode)
        with s.scratch.labels() as buf:
            b0 = s.scratch.label(None, lv, _engine.CONNECT_FACES, _engine.REGION_INSIDE, buf)
            k_out = s.scratch.label(None, lv, _engine.CONNECT_FULL, _engine.REGION_OUTSIDE, buf)
            border = s.scratch.records(k_out, buf)[4]
    enclosed = int(np.count_nonzero(~border))
    euler = cells[0] - cells[1] + cells[2] - cells[3]
    if len(tables) == 3:
        return Topology(b0, b0 + enclosed - euler, enclosed, cells, [t.size for t in tables])
    if b0 - euler != enclosed:
        raise RuntimeError("betti: %d holes by labelling the outside, but b0 - euler = %d - %d" % (enclosed, b0, euler))
    return Topology(b0, enclosed, 0, cells, [t.size for t in tables])
