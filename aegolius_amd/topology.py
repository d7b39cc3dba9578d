"""Topology of a solid on a grid, on the GPU: connected components with their sizes, boxes and mass properties, enclosed
cavities and through-holes (kernels: csrc/sdfk_topology.inc).

    from aegolius_amd import topology, redistance
    c = topology.from_geometry(geometry, (2, 2, 2), (257, 257, 257))     # or topology.label(field or geometry, axes)
    c.count, c.sizes, c.box(c.largest())                                 # islands, their points, the body's box
    body = c.field(keep=[c.largest()])                                   # a DeviceField: the body without its debris
    d = redistance.redistance(body, axes)
    t = topology.betti(geometry, axes)                                   # t.components, t.tunnels, t.cavities, t.euler
    m = c.moments()                                                      # every component's integer moments, one pass
    m.volumes, m.centroids, m.properties(c.largest(), density=7850.0)    # (K,), (K, D), a moments.MassProperties
    v = topology.cavities(geometry, axes)                                # the enclosed voids: v.count, v.volumes, v.centroids

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

Component moments (the kernel, `ComponentMoments` and tests/component_moments_reference.py implement exactly this). The
integer sums of component k are taken over all points p with label[p] == k, i_a the index of p on axis a, in this order:

    3-D: (N, I0, I1, I2, I00, I01, I02, I11, I12, I22)      ten sums of 1, i_a, i_a i_b
    2-D: (N, I0, I1, I00, I01, I11)                         six sums

as uint64; points with label -1 belong to no component, N equals sizes[k]. The moments of `moments.py` at samples = 1
(odd lattice coordinate u = 2 i + 1) follow on the host in Python ints, U_a = 2 I_a + N and U_ab = 4 I_ab + 2 I_a + 2 I_b
+ N, and with them MassProperties(M, lo, step, shape, 1, level, density, near_cells=0) is the component's mass properties,
text and formulas of `moments.py` unchanged: the solid is the union of the grid cells whose centre point belongs to the
component. World quantities need uniform tables by the rule of moments._uniform (tested on the float64 tables the caller
gave); the sums exist for any tables. No wrap: with n points and axis lengths d_a a call is refused before any launch when
n (d_a - 1)(d_b - 1) >= 2^63 for some a <= b; below that no 64-bit sum can wrap, whatever the order of addition (with
n <= 2^31 - 1 that refuses long, thin grids only). Integer adds only: two calls return identical bits.

A geometry whose tree lowers to one program is evaluated to one inside bit per point: no field and no coordinate array
exist. A staged tree (grid operators such as conv_averaging) is evaluated to a resident field first, as in `mesh`.

Not here: more than 2^31 - 1 points; more than one GPU; periodic grids; sub-sampled (samples > 1) per-component moments
(`field(keep=[k])` is a DeviceField, which `moments` does not take: it samples geometries); attributing a cavity to the
component that encloses it. The layers of a plane stack labelled as separate 2-D problems, with the links between
consecutive layers, are in `layers`.
"""
import numpy as np

from . import _engine
from .mesh import _grid_of, _is_geometry, _level, _points, _tables
from .occupancy import _axes as _given_axes

CONNECTIVITY = ("faces", "full")
REGION = ("inside", "outside")
MAX_POINTS = 2 ** 31 - 1


def sums_can_wrap(shape):
    """True when a 64-bit moment sum could wrap on a grid of that shape: n (d_a - 1)(d_b - 1) >= 2^63 for some pair of
    axes, n the number of points — that is n (d_max - 1)^2 >= 2^63. Python ints: exact."""
    dims = [int(d) for d in shape]
    n = 1
    for d in dims:
        n *= d
    return n * (max(dims) - 1) ** 2 >= 2 ** 63


def _check_wrap(shape):
    if sums_can_wrap(shape):
        raise ValueError("component moments: a 64-bit sum could wrap on the grid %s (points x (longest axis - 1)^2 >= 2^63)"
                         % "x".join(str(int(d)) for d in shape))


def _keep_mask(count, keep):
    """`keep` -> (count,) bool: every id (None), a sequence of ids, or a boolean array of length count."""
    mask = np.ones(count, dtype=bool)
    if keep is not None:
        k = np.asarray(keep)
        if k.dtype == bool:
            if k.shape != (count,):
                raise ValueError("keep: a boolean array has one entry per component (%d); got shape %r" % (count, k.shape))
            mask = k.copy()
        else:
            ids = np.asarray(keep, dtype=np.int64).ravel()
            if ids.size and (ids.min() < 0 or ids.max() >= count):
                raise ValueError("keep: ids are 0 .. %d" % (count - 1))
            mask = np.zeros(count, dtype=bool)
            mask[ids] = True
    return mask


def index_moments(row):
    """A row of integer sums (N, I_a, I_ab; ten or six entries) -> the tuple M of moments.py at samples = 1 as Python ints:
    U_a = 2 I_a + N, U_ab = 4 I_ab + 2 I_a + 2 I_b + N."""
    from .moments import PAIRS_2D, PAIRS_3D                     # (here: the package does not import `moments` by itself)
    row = [int(v) for v in row]
    if len(row) not in (6, 10):
        raise ValueError("a row of moment sums has 6 (2-D) or 10 (3-D) entries; got %d" % len(row))
    d = 3 if len(row) == 10 else 2
    N, first = row[0], row[1:1 + d]
    second = [4 * Iab + 2 * first[a] + 2 * first[b] + N for (a, b), Iab in zip(PAIRS_3D if d == 3 else PAIRS_2D, row[1 + d:])]
    return (N,) + tuple(2 * Ia + N for Ia in first) + tuple(second)


class ComponentMoments:
    """The integer moments of K components on one grid (the module text states the sums): `sums` (K, 10) or (K, 6) uint64,
    `count`, `dims`, `shape`, `axes` (float64 tables), `level`. Made by Components.moments(), label(..., moments=True) and
    cavities(), or on the host from any `sums` and axis tables. volumes, centroids, properties and total_properties are
    world quantities: they raise moments._uniform's ValueError on non-uniform tables; sums, index_moments and total do
    not."""

    def __init__(self, sums, tables, level=0.0):
        self.axes = tuple(np.asarray(t, dtype=np.float64).ravel() for t in tables)
        self.dims = len(self.axes)
        if self.dims not in (2, 3):
            raise ValueError("ComponentMoments: 2 or 3 axis tables; got %d" % self.dims)
        width = 10 if self.dims == 3 else 6
        sums = np.asarray(sums)
        if sums.ndim != 2 or sums.shape[1] != width or sums.dtype.kind not in "ui":
            raise ValueError("ComponentMoments: %d-D sums are an integer array of shape (K, %d); got %s %r"
                             % (self.dims, width, sums.dtype, sums.shape))
        if sums.dtype.kind == "i" and sums.size and sums.min() < 0:
            raise ValueError("ComponentMoments: sums are not negative")
        self.sums = np.ascontiguousarray(sums, dtype=np.uint64)
        self.count = int(self.sums.shape[0])
        self.shape = tuple(int(t.size) for t in self.axes)
        self.level = level

    def __len__(self):
        return self.count

    def __repr__(self):
        return "ComponentMoments(%d components, grid %s)" % (self.count, "x".join(map(str, self.shape)))

    def index_moments(self, k):
        """The tuple M of moments.py (samples = 1) of component k, Python ints."""
        return index_moments(self.sums[range(self.count)[k]])

    def total(self, keep=None):
        """The sums of the rows of the kept components (`keep` as for Components.field) -> a tuple of Python ints: the
        integer sums of the union of those components."""
        mask = _keep_mask(self.count, keep)
        return tuple(sum(int(v) for v in column) for column in self.sums[mask].T)

    def select(self, keep):
        """The ComponentMoments of the kept components alone, in their order."""
        return ComponentMoments(self.sums[_keep_mask(self.count, keep)], self.axes, self.level)

    def _uniform(self):
        from .moments import _uniform
        return _uniform(self.axes)

    def _properties(self, row, density):
        from .moments import MassProperties, _density
        lo, step = self._uniform()
        return MassProperties(index_moments(row), lo, step, self.shape, 1, self.level, _density(density), 0)

    def properties(self, k, density=1.0):
        """The mass properties of component k -> moments.MassProperties (samples = 1, near_cells = 0)."""
        return self._properties(self.sums[range(self.count)[k]], density)

    def total_properties(self, keep=None, density=1.0):
        """The mass properties of the union of the kept components -> moments.MassProperties."""
        return self._properties(self.total(keep), density)

    @property
    def volumes(self):
        """(K,) float64: N times the cell volume (area in 2-D)."""
        _lo, step = self._uniform()
        return self.sums[:, 0].astype(np.float64) * float(np.prod(step))

    @property
    def centroids(self):
        """(K, D) float64: centroid_a = a_0 + (I_a / N) h_a (NaN for an empty row)."""
        _lo, step = self._uniform()
        first = np.array([a[0] for a in self.axes])
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = self.sums[:, 1:1 + self.dims].astype(np.float64) / self.sums[:, :1].astype(np.float64)
        return first + mean * step


class Components:
    """The components of one labelling: `count` K, `first` (K,) int64, `sizes` (K,) int64, `lower` / `upper` (K, D) int32,
    `border` (K,) bool as host arrays; `shape`, `connectivity`, `region`, `level`, `axes` (the float32 tables);
    `labels`: the device-resident int32 ids (an _engine.DeviceBuffer of prod(shape) entries, -1 off the region), None
    after label(..., labels=False) or free(). The buffer is freed with the object. moments(): the ComponentMoments."""

    def __init__(self, records, labels, tables, connectivity, region, level, device, given=None):
        self.first, self.sizes, self.lower, self.upper, self.border = records
        self.count = int(len(self.first))
        self.labels = labels
        self.axes = tuple(tables)
        self.shape = tuple(int(t.size) for t in tables)
        self.connectivity, self.region, self.level, self.device = connectivity, region, level, device
        self._given = tuple(given) if given is not None else self.axes     # the caller's tables in float64, for moments()
        self._moments = None

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
        mask = _keep_mask(self.count, keep)
        labels = self._labels()
        return _engine.label_field(labels, int(np.prod(self.shape)), mask, np.float32(inside), np.float32(outside), self.device)

    def moments(self):
        """The integer moments of every component -> ComponentMoments: one more pass over the labels, made once and kept
        with the object (label(..., moments=True) makes them inside the call, before labels=False drops the array).
        ValueError when the labels were dropped or freed before, or when a sum could wrap on this grid (the module text)."""
        if self._moments is None:
            labels = self._labels()
            _check_wrap(self.shape)
            self._moments = ComponentMoments(_engine.label_moments(labels, self.shape, self.count), self._given, self.level)
        return self._moments


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
def label(source, axes, level=0.0, connectivity="faces", region="inside", labels=True, timings=None, moments=False):
    """The connected components of the region of {source <= level} on the grid of `axes` -> Components.
    `source`: a host array of prod(shape) values in C order, a DeviceField, or a geometry (any tree create() evaluates);
    `axes`: as for mesh.isosurface / mesh.contour (2 or 3 tables, or a generate_grid array); `labels=False` drops the
    device label array once the records are made. At most 2^31 - 1 points (labels are int32). `timings`: a dict that
    receives device-event milliseconds of bits / init / merge / compress / number. `moments=True` takes the component
    moments inside the call, before `labels=False` drops the array: Components.moments() then returns them."""
    return _label(source, _axes(axes), _grid_of(axes), level, connectivity, region, labels, timings, moments, axes)


def _label(source, tables, grid, level, connectivity, region, labels, timings, moments=False, given=None):
    lv = _level(level)
    conn, reg = _choice(connectivity, CONNECTIVITY, "connectivity"), _choice(region, REGION, "region")
    if moments:
        _check_wrap([t.size for t in tables])
    if given is not None:
        given = _given_axes(given)[0]                          # the caller's tables in float64: what moments._uniform tests
    with _Session(source, grid, tables, lv) as s:
        buf = s.scratch.labels()
        try:
            count = s.scratch.label(s.source, lv, conn, reg, buf, s.mode, timings)
            records = s.scratch.records(count, buf)
            found = Components(records, buf, tables, connectivity, region, lv, s.scratch.device, given)
            if moments:
                found.moments()
        except BaseException:
            buf.free()
            raise
        if not labels:
            found.free()
        return found


def from_geometry(geometry, size, resolution, level=0.0, connectivity="faces", region="inside", labels=True, moments=False):
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
    return _label(geometry, _axes(axes), grid, level, connectivity, region, labels, None, moments, axes)


def cavities(source, axes, level=0.0):
    """The enclosed voids of {source <= level} with their moments -> ComponentMoments (count, volumes, centroids, ...):
    the components of the outside under "full" that do not touch the border of the grid — the labelling `betti` counts
    for b2 (3-D) and for the holes (2-D). No label array outlives the call."""
    found = label(source, axes, level, connectivity="full", region="outside", labels=False, moments=True)
    return found.moments().select(~found.border)


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
