"""Layer graphs of a plane stack, on the GPU: the pieces of every layer, which of them have nothing beneath, and how the
pieces of one layer connect to those of the next (kernels: csrc/sdfk_layers.inc).

    from aegolius_amd import layers
    g = layers.from_geometry(geometry, (2, 2, 2), (257, 257, 257))       # z-layers on generate_grid's tables
    g = layers.graph(geometry or field, (U, V), heights, normal=2)       # or: any stack slices.stack takes, or its field
    g.islands(), g.overhang, g.parents(c), g.children(c)                 # pieces without support; unsupported points; links
    g.per_layer().overhang, g.overhang_area(), g.events().merges
    g.moments().centroids[g.islands()]                                   # where the islands are, in (h, a, b) units
    support = g.field(keep=g.islands())                                  # a DeviceField of the islands alone

Definitions (the kernels and tests/layers_reference.py implement exactly this):
  * Grid. Heights H (L >= 2) and in-plane tables U (nu >= 2), V (nv >= 2), strictly increasing as float32. The layer is the
    slowest axis: the linear index of point (l, i, j) is p = (l nu + i) nv + j, as in `topology` and `slices`. At most
    2^31 - 1 points, because labels are int32.
  * Inside. `topology`'s rule: f <= level as a comparison of selection keys, NaN outside.
  * Region. Only the inside points are labelled; there is no `outside` region here.
  * Layer components. The components of the inside points of one layer under in-plane connectivity: "faces" (4
    neighbours) or "full" (8). Two points of different layers are never joined. A component's name is the smallest linear
    index among its points; ids 0 .. K - 1 run by ascending name, so ids ascend with the layer, and `layer_offsets`
    (L + 1,) int64 bounds the ids of every layer: layer l holds the ids layer_offsets[l] .. layer_offsets[l + 1] - 1.
  * Records per component, as `topology` has them: `first`, `sizes`, `lower` / `upper` (K, 3) int32 with lower[:, 0] ==
    upper[:, 0] == the layer, and `border`: true when a point of the component lies on one of the four in-plane edges of
    the rectangle (i = 0, i = nu - 1, j = 0 or j = nv - 1). Lying in the first or last layer does not count.
  * Links. For a component c of layer l >= 1 and a component q of layer l - 1, overlap(c, q) is the number of columns
    (i, j) with label[l, i, j] = c and label[l - 1, i, j] = q — the same column only, whatever the in-plane connectivity.
    There is a link where overlap > 0. The link list `child`, `parent`, `overlap` (E,) int64 is sorted by (child, parent).
  * Per component: supported[c] = the sum of overlap(c, q) over q, the points with material directly beneath;
    overhang[c] = sizes[c] - supported[c]. Components of layer 0 have supported = 0 by definition: they are the base.
  * Islands. A component of a layer >= 1 with supported == 0.
Every output is an integer and independent of scheduling: two calls agree bit for bit, and the GPU agrees with the
reference, with no relabelling.

A geometry is seen through the frame (`slices.Frame.apply`: one coordinate transform in front of its unchanged program),
exactly the field `slices.stack` slices, and is evaluated to one inside bit per point: no field exists. The labelling is
`topology`'s with a merge pass that stays in the plane; the link pass finds, per 32-point word, the stretches where a
layer and the one beneath are both inside — a candidate (child, parent, length) each — and adds up `supported`. The
candidates are combined to the sorted link list on the host, in integers.

Not here: an outside region per layer (the holes of a layer); links through diagonal columns or with a horizontal reach
(a self-supporting angle); support-structure generation; device-side deduplication of the link candidates (they cross
PCIe once, 12 bytes each); sub-sampled (samples > 1) measures; staged trees (refused, as in `slices`); more than one GPU.
"""
import collections

import numpy as np

from . import _engine
from .mesh import _is_geometry, _level, _points
from .slices import Frame, _frame, _prepare, _table
from .topology import CONNECTIVITY, MAX_POINTS, Components, _choice

LayerTotals = collections.namedtuple("LayerTotals", "components inside supported overhang islands")
LayerEvents = collections.namedtuple("LayerEvents", "births merges splits ends")


def combine(child, parent, length):
    """Link candidates (one per stretch; a pair may come more than once, in any order) -> child, parent, overlap (E,) int64,
    unique pairs sorted by (child, parent), overlap the sum of the pair's lengths. Integer work only."""
    child, parent = np.asarray(child, dtype=np.int64), np.asarray(parent, dtype=np.int64)
    key = (child << 32) | parent
    order = np.argsort(key, kind="stable")
    key = key[order]
    starts = np.flatnonzero(np.r_[True, key[1:] != key[:-1]]) if key.size else np.zeros(0, dtype=np.int64)
    overlap = np.add.reduceat(np.asarray(length, dtype=np.int64)[order], starts) if key.size else np.zeros(0, dtype=np.int64)
    key = key[starts]
    return key >> 32, key & 0xffffffff, overlap.astype(np.int64)


class LayerGraph(Components):
    """The layer components of a stack and their links. A topology.Components of the layered labels — `count` K, `first`,
    `sizes`, `lower`, `upper`, `border` (in-plane), `labels`, labels_host(), field(keep=), box(k), moments(), free() work
    unchanged; `axes` = (H, U, V) float32 — and `layers` L, `layer_offsets` (L + 1,), `layer_of` (K,), `child` / `parent` /
    `overlap` (E,), `supported` / `overhang` (K,), all int64; `frame` (None for a field source)."""

    def __init__(self, records, labels, tables, connectivity, level, device, links, supported, frame=None, given=None):
        Components.__init__(self, records, labels, tables, connectivity, "inside", level, device, given)
        self.frame = frame
        self.layers = self.shape[0]
        self.layer_of = self.lower[:, 0].astype(np.int64)
        self.layer_offsets = np.searchsorted(self.layer_of, np.arange(self.layers + 1)).astype(np.int64)
        self.child, self.parent, self.overlap = links
        self.supported = np.asarray(supported, dtype=np.int64)
        self.overhang = self.sizes - self.supported

    def __repr__(self):
        return "LayerGraph(%d layers, %d components, %d links, %d islands, %s)" % (self.layers, self.count, len(self.child),
                                                                                   len(self.islands()), self.connectivity)

    def islands(self):
        """Ids of the components of a layer >= 1 with nothing beneath, ascending."""
        return np.flatnonzero((self.supported == 0) & (self.layer_of >= 1)).astype(np.int64)

    def parents(self, c):
        """Ids of the components of the layer below that component c rests on, ascending."""
        c = range(self.count)[c]
        return self.parent[np.searchsorted(self.child, c, "left"):np.searchsorted(self.child, c, "right")].copy()

    def children(self, c):
        """Ids of the components of the layer above that rest on component c, ascending."""
        return np.sort(self.child[self.parent == range(self.count)[c]])

    def per_layer(self):
        """(L,) int64 arrays: components, inside points, supported points, overhang points and islands of every layer ->
        LayerTotals(components, inside, supported, overhang, islands)."""
        components = np.bincount(self.layer_of, minlength=self.layers).astype(np.int64)
        inside = np.zeros(self.layers, dtype=np.int64)
        supported = np.zeros(self.layers, dtype=np.int64)
        np.add.at(inside, self.layer_of, self.sizes)
        np.add.at(supported, self.layer_of, self.supported)
        islands = np.bincount(self.layer_of[self.islands()], minlength=self.layers).astype(np.int64)
        return LayerTotals(components, inside, supported, inside - supported, islands)

    def events(self):
        """Ids, ascending -> LayerEvents(births: no parent and layer >= 1 (the islands), merges: two or more parents, splits:
        two or more children, ends: no child and layer < L - 1)."""
        parents = np.bincount(self.child, minlength=self.count)
        children = np.bincount(self.parent, minlength=self.count)
        ids = lambda mask: np.flatnonzero(mask).astype(np.int64)  # noqa: E731
        return LayerEvents(ids((parents == 0) & (self.layer_of >= 1)), ids(parents >= 2), ids(children >= 2),
                           ids((children == 0) & (self.layer_of < self.layers - 1)))

    def overhang_area(self):
        """(L,) float64: the overhang points of every layer times du dv. ValueError for non-uniform U or V (the rule of
        moments._uniform, tested on the float64 tables the caller gave)."""
        from .moments import _uniform
        _lo, step = _uniform(self._given[1:])
        return self.per_layer().overhang.astype(np.float64) * float(step[0] * step[1])


class _Source:
    """The scratch of one call and its source on the device: a program (inside bits, no field), the caller's resident
    field, or an uploaded host array."""

    def __init__(self, source, tables):
        from ._eval import config
        self.own = self.scratch = None
        self.mode = config.mode
        _engine.require_gpu()
        try:
            if isinstance(source, (_engine.Program, _engine.DeviceField)):
                if isinstance(source, _engine.DeviceField):
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


def _check(source, axes, heights, normal, level, connectivity):
    """Every argument check, before anything asks for the GPU -> (program or field, tables (H, U, V), level, connectivity
    index, frame or None)."""
    conn = _choice(connectivity, CONNECTIVITY, "connectivity")
    if len(axes) != 2:
        raise ValueError("axes: the two in-plane tables (U, V); got %d" % len(axes))
    tables = [_table(heights, "heights", 2), _table(axes[0], "axis U", 2), _table(axes[1], "axis V", 2)]
    n = int(np.prod([t.size for t in tables], dtype=np.int64))
    if n > MAX_POINTS:
        raise ValueError("the stack spans %s = %d points; labels are int32: at most 2^31 - 1 points"
                         % ("x".join(str(t.size) for t in tables), n))
    if _is_geometry(source):
        prog, tables, lv, frame = _prepare(source, axes, heights, normal, level)       # (refuses a staged tree)
        return prog, tables, lv, conn, frame
    if isinstance(normal, Frame):
        raise ValueError("a Frame goes with a geometry: a field holds the values of its own stack already")
    _frame(normal)
    lv = _level(level)
    if _points(source) != n:
        raise ValueError("the field has %d values; the stack spans %s = %d points"
                         % (_points(source), "x".join(str(t.size) for t in tables), n))
    return source, tables, lv, conn, None


# ---- public interface -------------------------------------------------------------------------------------------------------
def graph(source, axes, heights, normal=2, level=0.0, connectivity="faces", labels=True, timings=None):
    """The layer graph of {source <= level} on the stack of `heights` and `axes` = (U, V) -> LayerGraph.
    `source`: a geometry, seen through slices' frame of `normal` (the coordinate axis 0, 1, 2 or a Frame) — the field
    slices.stack slices; or a host array or DeviceField of L nu nv values in (H, U, V) order (a Frame together with a
    field is a ValueError). A staged tree is refused, as in `slices`. `labels=False` drops the device label array once
    records and links are made. `timings`: a dict that receives device-event milliseconds of bits / init / merge /
    compress / number (the labelling), records, links (count, scan, `supported`) and candidates (emit), each with its
    download; host milliseconds of prepare (the checks and the lowering of a geometry), allocate (scratch, labels, an
    uploaded field), label_wall (the whole labelling call, the five passes and the host's share) and combine; and the
    numbers `candidate_count` and `link_count`."""
    import time

    def host(name, since):
        if timings is not None:
            timings[name] = timings.get(name, 0.0) + (time.perf_counter() - since) * 1e3
        return time.perf_counter()
    t0 = time.perf_counter()
    src, tables, lv, conn, frame = _check(source, axes, heights, normal, level, connectivity)
    given = [np.asarray(heights, dtype=np.float64).ravel()] + [np.asarray(a, dtype=np.float64).ravel() for a in axes]
    t0 = host("prepare", t0)
    with _Source(src, tables) as s:
        buf = s.scratch.labels()
        t0 = host("allocate", t0)
        try:
            count = s.scratch.layer_label(s.source, lv, conn, buf, s.mode, timings)
            host("label_wall", t0)
            timer = _engine.Timer(timings)
            timer.mark("start")
            records = s.scratch.layer_records(count, buf)
            timer.mark("records")
            candidates, supported = s.scratch.layer_link_count(count, buf)
            timer.mark("links")
            child, parent, length = s.scratch.layer_link_candidates(count, buf, candidates)
            timer.mark("candidates")
            timer.finish()
            t0 = time.perf_counter()
            links = combine(child, parent, length)
            host("combine", t0)
            if timings is not None:
                timings["candidate_count"], timings["link_count"] = candidates, int(links[0].size)
            found = LayerGraph(records, buf, tables, connectivity, lv, s.scratch.device, links, supported, frame, given)
        except BaseException:
            buf.free()
            raise
        if not labels:
            found.free()
        return found


def from_geometry(geometry, size, resolution, normal=2, level=0.0, connectivity="faces", labels=True, timings=None):
    """graph() on the grid generate_grid(size, resolution) spans (3 sizes), the tables picked as slices.from_geometry picks
    them: for normal k the table of axis k becomes the heights and the two others (U, V) in cyclic order; for a Frame the
    three tables are (heights, U, V) as they come."""
    from .cores.helper_functions import grid_axes
    if len(size) != 3:
        raise ValueError("from_geometry: size has 3 entries")
    if not _is_geometry(geometry):
        raise ValueError("from_geometry takes a geometry; graph() takes fields")
    axes, _ = grid_axes(size, resolution)
    frame = _frame(normal)
    k = 0 if frame is normal else int(normal)
    return graph(geometry, (axes[(k + 1) % 3], axes[(k + 2) % 3]), axes[k], normal, level, connectivity, labels, timings)
