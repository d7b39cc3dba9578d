"""Layer graphs on the GPU (aegolius_amd.layers; kernels: csrc/sdfk_layers.inc) against the numpy reference
(tests/layers_reference.py) on the same inside bits. Every answer is an integer and every assertion exact equality: labels,
records, layer offsets, links, supported and overhang counts, islands, events and layer totals — on hand-made patterns as
resident fields, on geometries through the bits path against the field path, and on shapes whose graph is known; two calls
agree bit for bit, and the consumers of a labelling (moments, label fields) work on the layered labels."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import aegolius_amd.cores as ns  # noqa: E402
import component_moments_reference as CM  # noqa: E402
import layers_reference as LR  # noqa: E402
from aegolius_amd import _engine, layers, mesh, slices  # noqa: E402
from aegolius_amd._eval import config  # noqa: E402

pytestmark = pytest.mark.gpu

CONNECTIVITY = ("faces", "full")


def _lin(lo, hi, n):
    return (np.linspace(lo, hi, n) + 0.0).astype(np.float32)


def _nonuniform(n, seed):
    rng = np.random.default_rng(seed)
    a = np.unique(np.sort(rng.uniform(-1.0, 1.0, 4 * n)).astype(np.float32))
    return np.ascontiguousarray(a[::4][:n] + np.float32(0.0))


def _uniform(*shape):
    return tuple(_lin(-1, 1, s) for s in shape)


# (H, U, V): the smallest grid; several layers inside one word; rows of one word, one word and a bit, two words, with layers
# of 288 / 297 / 576 points so that the word one layer below is unaligned; general unaligned rows; three tiles, layers cut by
# tile seams; non-uniform tables
GRIDS = {
    "2x2x2": _uniform(2, 2, 2),
    "3x5x7": _uniform(3, 5, 7),
    "5x9x32": _uniform(5, 9, 32),
    "5x9x33": _uniform(5, 9, 33),
    "5x9x64": _uniform(5, 9, 64),
    "4x33x40": _uniform(4, 33, 40),
    "9x40x48": _uniform(9, 40, 48),
    "3x40x33_nonuniform": (_nonuniform(3, 1), _nonuniform(40, 2), _nonuniform(33, 3)),
}


# ---- patterns: boolean arrays (True = inside) -----------------------------------------------------------------------------
def _serpentine2d(rows, cols):
    """Every second row is inside; the rows between hold one connector, alternately at the right and at the left end."""
    m = np.zeros((rows, cols), dtype=bool)
    m[0::2] = True
    for r in range(1, rows - 1, 2):
        m[r, cols - 1 if (r // 2) % 2 == 0 else 0] = True
    return m


def serpentine(shape):
    """A serpentine on every second layer — one in-plane component whose path visits every row; the layers between hold
    one point, alternately over the path's end and its start: a component of one point that links two serpentines."""
    m = np.zeros(shape, dtype=bool)
    flat = _serpentine2d(shape[1], shape[2])
    last = (shape[1] - 1) // 2 * 2
    end = (last, shape[2] - 1 if (last // 2) % 2 == 1 else 0)
    m[0::2] = flat
    for layer in range(1, shape[0] - 1, 2):
        m[(layer,) + (end if (layer // 2) % 2 == 0 else (0, 0))] = True
    return m


def comb(shape):
    """Teeth along j that meet only in a layer's last row, on every second layer; the layers between hold that row alone."""
    m = np.zeros(shape, dtype=bool)
    m[0::2, :, 0::2] = True
    m[:, -1, :] = True
    return m


def staircase(shape):
    """Diagonals over (i, j), shifted by one from layer to layer: joined under full, single points under faces, and no
    point has one beneath."""
    idx = np.indices(shape)
    return idx[2] == (idx[1] + idx[0]) % shape[2]


def patterns(key):
    shape = tuple(t.size for t in GRIDS[key])
    out = {
        "all_inside": np.ones(shape, dtype=bool),
        "all_outside": np.zeros(shape, dtype=bool),
        "checkerboard": np.indices(shape).sum(axis=0) % 2 == 0,
        "comb": comb(shape),
        "staircase": staircase(shape),
        "serpentine": serpentine(shape),
    }
    for density in (0.31, 0.59):
        rng = np.random.default_rng(int(1000 * density) + 3)
        out["noise_%g" % density] = rng.random(shape) < density
    return out


def _field(mask):
    return np.where(mask, np.float32(-1), np.float32(1)).astype(np.float32)


# ---- comparison -----------------------------------------------------------------------------------------------------------------
RECORDS = ("first", "sizes", "lower", "upper", "border")
ARRAYS = ("layer_offsets", "layer_of", "child", "parent", "overlap", "supported", "overhang")


def _same_graph(got, want, what, labels=True):
    assert got.count == want.count, (what, got.count, want.count)
    if labels:
        np.testing.assert_array_equal(got.labels_host(), want.labels, err_msg=str(what))
    for name in RECORDS + ARRAYS:
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg="%s %s" % (what, name))
    np.testing.assert_array_equal(got.islands(), LR.islands(want), err_msg=str(what))
    for g, w in zip(got.events(), LR.events(want)):
        np.testing.assert_array_equal(g, w, err_msg="%s events" % (what,))
    for g, w in zip(got.per_layer(), LR.per_layer(want)):
        np.testing.assert_array_equal(g, w, err_msg="%s per_layer" % (what,))


_REFERENCE = {}


def _reference(key, name, connectivity):
    """The reference graph of a pattern: made once, shared by the tests, never changed."""
    at = (key, name, connectivity)
    if at not in _REFERENCE:
        _REFERENCE[at] = LR.graph(patterns(key)[name], connectivity)
    return _REFERENCE[at]


@pytest.mark.parametrize("key", sorted(GRIDS))
def test_patterns_equal_the_reference(engine, key):
    H, U, V = GRIDS[key]
    for name, mask in patterns(key).items():
        dev = _engine.DeviceField.from_host(_field(mask), config.device)
        try:
            for connectivity in CONNECTIVITY:
                got = layers.graph(dev, (U, V), H, connectivity=connectivity)
                _same_graph(got, _reference(key, name, connectivity), (key, name, connectivity))
                got.free()
        finally:
            dev.free()


def test_patterns_are_what_they_claim():
    """The stress patterns have the structure they are there for (reference only)."""
    s = _reference("9x40x48", "serpentine", "faces")
    assert s.count == 9 and LR.islands(s).size == 0 and s.sizes[0] > 40 * 48 // 2 and s.overlap.tolist() == [1] * 8
    c = _reference("9x40x48", "comb", "faces")
    assert c.count == 9 and c.first[0] == 0 and c.overhang[1::2].tolist() == [0] * 4
    d = _reference("9x40x48", "staircase", "faces")
    assert d.count == 9 * 40 and d.child.size == 0 and LR.islands(d).size == 8 * 40
    assert _reference("9x40x48", "staircase", "full").count == 9              # (one diagonal per layer)


# ---- geometries: the bits path against the field path -------------------------------------------------------------------
def _oblique():
    u = np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)
    n = np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0)
    v = np.cross(n, u)
    return slices.Frame((0.1, -0.05, 0.2), u, v / np.linalg.norm(v))


STACK = (_lin(-0.6, 0.6, 9), _lin(-1, 1, 40), _lin(-1, 1, 48))                  # 9 layers 0.15 apart


def _moved(geo, to):
    geo.move(to)
    return geo


def _union(*parts):
    out = parts[0]
    for p in parts[1:]:
        out = ns.CombineGeometry("UNION").combine(out, p)
    return out


def sphere_over_plate():
    """Seen along z: a plate in layer 0 alone, and a sphere of radius 0.33 around z = 0.15 that fills layers 3 .. 7."""
    return _union(_moved(ns.Box(1.6, 1.6, 0.1), (0, 0, -0.6)), _moved(ns.Sphere(0.33), (0, 0, 0.15)))


def upright_torus():
    """A ring of radius 0.5 and tube radius 0.17 in the xz plane. Seen along z it starts in layer 0 (z = -0.6), is one piece
    while |z| > 0.33 and two pieces in the five layers between."""
    t = ns.Torus(0.5, 0.17)
    t.rotate(np.pi / 2, (1, 0, 0))
    return t


def pillars_and_bridge():
    """Seen along z: two pillars in layers 0 .. 5 (z up to 0.2), a bridge over both in layers 6 and 7 (z in [0.25, 0.55])."""
    return _union(_moved(ns.Box(0.3, 0.3, 0.85), (-0.5, 0, -0.225)), _moved(ns.Box(0.3, 0.3, 0.85), (0.5, 0, -0.225)),
                  _moved(ns.Box(1.3, 0.3, 0.3), (0, 0, 0.4)))


SHAPES = {"sphere_over_plate": sphere_over_plate, "upright_torus": upright_torus, "pillars_and_bridge": pillars_and_bridge}
NORMALS = {"axis0": 0, "axis1": 1, "axis2": 2, "oblique": _oblique()}


@pytest.mark.parametrize("normal", sorted(NORMALS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_geometry_path_equals_field_path_and_reference(engine, shape, normal):
    H, U, V = STACK
    frame = slices._frame(NORMALS[normal])
    co = mesh._grid_array([t.astype(np.float64) for t in STACK])
    field = np.asarray(frame.apply(SHAPES[shape]()).create(co), dtype=np.float32)
    mask = LR.R.inside(field).reshape(9, 40, 48)
    assert mask.any()
    for connectivity in CONNECTIVITY:
        want = LR.graph(mask, connectivity)
        by_bits = layers.graph(SHAPES[shape](), (U, V), H, normal=NORMALS[normal], connectivity=connectivity)
        by_field = layers.graph(field, (U, V), H, connectivity=connectivity)
        np.testing.assert_array_equal(by_bits.labels_host(), by_field.labels_host())
        _same_graph(by_bits, want, (shape, normal, connectivity, "bits"))
        _same_graph(by_field, want, (shape, normal, connectivity, "field"))
        assert by_bits.frame is frame or normal != "oblique"
        assert by_field.frame is None


@pytest.mark.parametrize("connectivity", CONNECTIVITY)
def test_shapes_whose_graph_is_known(engine, connectivity):
    """By the module's definitions a birth is a component of a layer >= 1 without a parent — the same set as the islands.
    The torus starts in layer 0, so its lowest piece is the base: no birth and no island, one split and one merge."""
    H, U, V = STACK
    g = layers.graph(sphere_over_plate(), (U, V), H, connectivity=connectivity)
    assert g.layer_offsets.tolist() == [0, 1, 1, 1, 2, 3, 4, 5, 6, 6]
    assert g.islands().tolist() == [1] and g.layer_of[1] == 3 and g.overhang[1] == g.sizes[1]
    ev = g.events()
    assert ev.births.tolist() == [1] and ev.merges.size == 0 and ev.splits.size == 0 and ev.ends.tolist() == [0, 5]
    assert g.border.tolist() == [False] * 6 and g.parents(2).tolist() == [1] and g.children(0).size == 0
    lo, hi = g.box(1)
    assert lo[0] == hi[0] == float(H[3])
    t = layers.graph(upright_torus(), (U, V), H, connectivity=connectivity)
    assert np.diff(t.layer_offsets).tolist() == [1, 1, 2, 2, 2, 2, 2, 1, 1]
    ev = t.events()
    assert ev.births.size == 0 and t.islands().size == 0 and ev.splits.tolist() == [1] and ev.merges.tolist() == [12]
    assert ev.ends.size == 0 and t.children(1).tolist() == [2, 3] and t.parents(12).tolist() == [10, 11]
    b = layers.graph(pillars_and_bridge(), (U, V), H, connectivity=connectivity)
    assert np.diff(b.layer_offsets).tolist() == [2] * 6 + [1, 1, 0]
    ev = b.events()
    assert ev.merges.tolist() == [12] and ev.births.size == 0 and ev.splits.size == 0 and ev.ends.tolist() == [13]
    assert b.supported[12] == b.sizes[10] + b.sizes[11] and b.overhang[12] == b.sizes[12] - b.sizes[10] - b.sizes[11] > 0
    assert b.overhang[13] == 0 and b.per_layer().overhang[1:].tolist() == [0] * 5 + [int(b.overhang[12]), 0, 0]
    du, dv = 2.0 / 39, 2.0 / 47
    np.testing.assert_allclose(b.overhang_area()[6], float(b.overhang[12]) * du * dv, rtol=1e-12)


def test_from_geometry_picks_the_tables_as_slices_does(engine):
    from aegolius_amd.cores.helper_functions import grid_axes
    axes, _ = grid_axes((1.2, 2, 2), (9, 40, 48))
    got = layers.from_geometry(sphere_over_plate(), (1.2, 2, 2), (9, 40, 48), normal=1, connectivity="full")
    want = layers.graph(sphere_over_plate(), (axes[2], axes[0]), axes[1], normal=1, connectivity="full")
    assert got.shape == (len(axes[1]), len(axes[2]), len(axes[0])) and got.count == want.count > 0
    np.testing.assert_array_equal(got.labels_host(), want.labels_host())
    for name in ARRAYS:
        np.testing.assert_array_equal(getattr(got, name), getattr(want, name))


# ---- determinism -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", CONNECTIVITY)
def test_deterministic_and_labels_false(engine, connectivity):
    H, U, V = GRIDS["9x40x48"]
    field = _field(patterns("9x40x48")["noise_0.31"])
    t = {}
    a = layers.graph(field, (U, V), H, connectivity=connectivity, timings=t)
    b = layers.graph(field, (U, V), H, connectivity=connectivity)
    c = layers.graph(field, (U, V), H, connectivity=connectivity, labels=False)
    np.testing.assert_array_equal(a.labels_host(), b.labels_host())
    for name in RECORDS + ARRAYS:
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name))
        np.testing.assert_array_equal(getattr(a, name), getattr(c, name))
    assert c.labels is None and c.count == a.count
    _same_graph(c, _reference("9x40x48", "noise_0.31", connectivity), "labels=False", labels=False)
    with pytest.raises(ValueError, match="dropped"):
        c.labels_host()
    assert t["candidate_count"] >= t["link_count"] == a.child.size > 0
    assert set(_engine.LABEL_PASSES) | {"prepare", "allocate", "label_wall", "records", "links", "candidates", "combine"} <= set(t)


# ---- existing consumers on the new labels ---------------------------------------------------------------------------------------
def test_moments_and_label_fields_of_the_layered_labels(engine):
    H, U, V = STACK
    g = layers.graph(sphere_over_plate(), (U, V), H)
    labels = g.labels_host()
    m = g.moments()
    np.testing.assert_array_equal(m.sums, CM.sums(labels, g.count))
    k = int(g.islands()[0])
    centre = m.centroids[k]                                                     # (h, a, b): the island lies under the sphere's centre
    assert centre[0] == pytest.approx(float(H[3]), abs=1e-6) and abs(centre[1]) < 0.03 and abs(centre[2]) < 0.03
    only = g.field(keep=g.islands())
    try:
        np.testing.assert_array_equal(only.numpy().reshape(labels.shape), np.where(labels == k, np.float32(-1), np.float32(1)))
    finally:
        only.free()
    noise = layers.graph(_field(patterns("4x33x40")["noise_0.59"]), GRIDS["4x33x40"][1:], GRIDS["4x33x40"][0], connectivity="full")
    labels = noise.labels_host()
    np.testing.assert_array_equal(noise.moments().sums, CM.sums(labels, noise.count))
    islands = noise.field(keep=noise.islands())
    try:
        np.testing.assert_array_equal(islands.numpy().reshape(labels.shape) < 0, np.isin(labels, noise.islands()))
    finally:
        islands.free()


def test_the_scratch_is_tagged_by_the_kind_of_labelling(engine):
    """The finishing calls refuse the other kind of labelling; relabelling the bits in the scratch needs no source."""
    H, U, V = GRIDS["4x33x40"]
    mask = patterns("4x33x40")["noise_0.31"]
    with _engine.DeviceField.from_host(_field(mask), config.device) as dev, _engine.LabelScratch((H, U, V), config.device) as scratch, \
            scratch.labels() as buf:
        k = scratch.layer_label(dev, 0.0, _engine.CONNECT_FACES, buf)
        assert k == LR.graph(mask, "faces").count
        with pytest.raises(_engine.SdfkError, match="layer labelling"):
            scratch.records(k, buf)
        k_full = scratch.layer_label(None, 0.0, _engine.CONNECT_FULL, buf)
        want = LR.graph(mask, "full")
        assert k_full == want.count
        candidates, supported = scratch.layer_link_count(k_full, buf)
        np.testing.assert_array_equal(supported, want.supported)
        with pytest.raises(_engine.SdfkError, match="link count"):
            scratch.layer_link_candidates(k_full, buf, candidates + 1)
        child, parent, length = scratch.layer_link_candidates(k_full, buf, candidates)
        assert child.size == candidates >= want.child.size
        for got, ref in zip(layers.combine(child, parent, length), (want.child, want.parent, want.overlap)):
            np.testing.assert_array_equal(got, ref)
        k3 = scratch.label(None, 0.0, _engine.CONNECT_FACES, _engine.REGION_INSIDE, buf)
        with pytest.raises(_engine.SdfkError, match="layer labelling"):
            scratch.layer_records(k3, buf)
        with pytest.raises(_engine.SdfkError, match="layer labelling"):
            scratch.layer_link_count(k3, buf)
