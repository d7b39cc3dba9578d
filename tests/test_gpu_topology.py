"""Topology queries on the GPU (aegolius_amd.topology; kernels: csrc/sdfk_topology.inc) against the numpy reference
(tests/topology_reference.py) on the same inside bits. Every answer is an integer and every assertion exact equality:
labels, counts, records, cell counts and Betti numbers, on hand-made patterns that stress the labelling (serpentines,
combs, staircases, checkerboards, noise on both sides of the percolation thresholds), on geometries through the bits
path against the field path, and on shapes whose Betti numbers are known."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import aegolius_amd.cores as ns  # noqa: E402
import topology_reference as R  # noqa: E402
import topology_shapes as S  # noqa: E402
from aegolius_amd import _engine, mesh, redistance, topology, workloads  # noqa: E402
from aegolius_amd._eval import config  # noqa: E402

pytestmark = pytest.mark.gpu

CONNECTIVITY = ("faces", "full")
REGION = ("inside", "outside")


def _lin(lo, hi, n):
    return (np.linspace(lo, hi, n) + 0.0).astype(np.float32)


def _nonuniform(n, seed):
    rng = np.random.default_rng(seed)
    a = np.unique(np.sort(rng.uniform(-1.0, 1.0, 4 * n)).astype(np.float32))
    return np.ascontiguousarray(a[::4][:n] + np.float32(0.0))


def _uniform(*shape):
    return tuple(_lin(-1, 1, s) for s in shape)


# the smallest shapes at which each mechanism can go wrong: one cell; words that straddle rows and layers; rows of exactly
# one word, one word and a bit, two words; rows longer than a word and unaligned; three tiles with layers split by tile
# seams; non-uniform tables; more than one tile in 2-D
GRIDS = {
    "2x2": _uniform(2, 2),
    "2x2x2": _uniform(2, 2, 2),
    "3x5x7": _uniform(3, 5, 7),
    "5x9x32": _uniform(5, 9, 32),
    "5x9x33": _uniform(5, 9, 33),
    "5x9x64": _uniform(5, 9, 64),
    "4x33x40": _uniform(4, 33, 40),
    "9x40x48": _uniform(9, 40, 48),
    "3x40x33_nonuniform": (_nonuniform(3, 1), _nonuniform(40, 2), _nonuniform(33, 3)),
    "130x130": _uniform(130, 130),
    "64x200": _uniform(64, 200),
    "64x64": _uniform(64, 64),
}
ALL_DENSITIES = ("3x5x7", "5x9x33", "9x40x48", "130x130")


# ---- patterns: boolean arrays (True = inside) -----------------------------------------------------------------------------
def _serpentine2d(rows, cols):
    """Every second row is inside; the rows between hold one connector, alternately at the right and at the left end:
    one component whose path visits every row, from the left and from the right in turn."""
    m = np.zeros((rows, cols), dtype=bool)
    m[0::2] = True
    for r in range(1, rows - 1, 2):
        m[r, cols - 1 if (r // 2) % 2 == 0 else 0] = True
    return m


def serpentine(shape):
    if len(shape) == 2:
        return _serpentine2d(*shape)
    # a serpentine on every second layer; the layers between hold one connector, alternately at the path's end and start
    m = np.zeros(shape, dtype=bool)
    flat = _serpentine2d(shape[1], shape[2])
    last = (shape[1] - 1) // 2 * 2
    end = (last, shape[2] - 1 if (last // 2) % 2 == 1 else 0)
    m[0::2] = flat
    for layer in range(1, shape[0] - 1, 2):
        m[(layer,) + (end if (layer // 2) % 2 == 0 else (0, 0))] = True
    return m


def comb(shape):
    """Teeth that meet only in the spine, the grid's last row: `first` is far from where the merges happen."""
    m = np.zeros(shape, dtype=bool)
    if len(shape) == 2:
        m[:, 0::2] = True
        m[-1, :] = True
        return m
    m[0::2, :, 0::2] = True                                    # teeth along j ...
    m[:, -1, 0::2] = True                                      # ... hang on teeth along i in the last plane ...
    m[-1, -1, :] = True                                        # ... which hang on the spine
    return m


def staircase(shape):
    """Diagonals over the last two axes, shifted by one from layer to layer: joined under full, single points under faces."""
    idx = np.indices(shape)
    a, b = idx[-2], idx[-1]
    shift = idx[0] if len(shape) == 3 else 0
    return b == (a + shift) % shape[-1]


def corners(shape):
    m = np.zeros(shape, dtype=bool)
    m[tuple(np.ix_(*[(0, s - 1) for s in shape]))] = True
    return m


def patterns(key):
    shape = tuple(t.size for t in GRIDS[key])
    out = {
        "all_inside": np.ones(shape, dtype=bool),
        "all_outside": np.zeros(shape, dtype=bool),
        "corners": corners(shape),
        "checkerboard": np.indices(shape).sum(axis=0) % 2 == 0,
        "comb": comb(shape),
        "staircase": staircase(shape),
    }
    if key in ("64x64", "9x40x48"):
        out["serpentine"] = serpentine(shape)
    for density in (0.2, 0.31, 0.5, 0.59, 0.8) if key in ALL_DENSITIES else (0.31, 0.59):
        rng = np.random.default_rng(int(1000 * density) + len(shape))
        out["noise_%g" % density] = rng.random(shape) < density
    return out


def _field(mask):
    return np.where(mask, np.float32(-1), np.float32(1)).astype(np.float32)


def _same_components(got, want, what):
    assert got.count == want.count, (what, got.count, want.count)
    np.testing.assert_array_equal(got.labels_host(), want.labels, err_msg=str(what))
    for name in ("first", "sizes", "lower", "upper", "border"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg="%s %s" % (what, name))


def _check_mask(field, tables, what):
    """Every query on one field (a host array) against the reference on its inside bits."""
    mask = R.inside(field).reshape([t.size for t in tables])
    dev = _engine.DeviceField.from_host(field, config.device)
    try:
        for connectivity in CONNECTIVITY:
            for region in REGION:
                want = R.label(mask if region == "inside" else ~mask, connectivity)
                got = topology.label(dev, tables, connectivity=connectivity, region=region)
                _same_components(got, want, (what, connectivity, region))
                got.free()
        assert topology.cell_counts(dev, tables) == R.cell_counts(mask), what
        t = topology.betti(dev, tables)
        b0, b1, b2, euler = R.betti(mask)
        assert (t.components, t.tunnels, t.cavities, t.euler) == (b0, b1, b2, euler), what
        assert (t.vertices, t.edges, t.faces, t.cubes) == R.cell_counts(mask) and t.shape == mask.shape
    finally:
        dev.free()


@pytest.mark.parametrize("key", sorted(GRIDS))
def test_patterns_equal_the_reference(engine, key):
    tables = GRIDS[key]
    for name, mask in patterns(key).items():
        _check_mask(_field(mask), tables, (key, name))


def test_patterns_are_what_they_claim():
    """The stress patterns have the structure they are there for (reference only)."""
    for shape in ((64, 64), (9, 40, 48)):
        s = R.label(serpentine(shape), "faces")
        assert s.count == 1 and s.sizes[0] > np.prod(shape) // 4
        c = R.label(comb(shape), "faces")
        assert c.count == 1 and c.first[0] == 0
        d = staircase(shape)
        assert R.label(d, "full").count < R.label(d, "faces").count == np.count_nonzero(d)
    assert R.label(staircase((9, 40, 48)), "full").count <= 2


def test_nan_counts_as_outside(engine):
    tables = GRIDS["4x33x40"]
    rng = np.random.default_rng(9)
    field = rng.uniform(-1, 1, [t.size for t in tables]).astype(np.float32)
    field[rng.random(field.shape) < 0.07] = np.nan
    assert np.isnan(field).sum() > 100
    for level in (0.0, 0.25):
        mask = R.inside(field, level)
        got = topology.label(field, tables, level=level, connectivity="full", region="outside")
        _same_components(got, R.label(~mask, "full"), ("nan", level))
        assert topology.cell_counts(field, tables, level) == R.cell_counts(mask)
    _check_mask(np.where(np.isnan(field), np.nan, np.sign(field)).astype(np.float32), tables, "nan sprinkled")


# ---- geometries: the bits path against the field path ---------------------------------------------------------------------
def _cloud():
    rng = np.random.default_rng(5)
    return ns.geom_3d.PointCloud3D(rng.uniform(-0.8, 0.8, (3, 300)))


SCENES = {
    "sphere": lambda: ns.Sphere(0.5),
    "cfg2_tree": lambda: workloads.cfg2_tree(ns),
    "cfg5_tree": lambda: workloads.cfg5_tree(ns),
    "sphere_union_64": lambda: workloads.sphere_union(ns, count=64, radius=0.12),      # chain mode, many components
    "point_cloud_300": _cloud,
}
GEOMETRY_GRIDS = ("2x2x2", "3x5x7", "5x9x32", "5x9x33", "5x9x64", "4x33x40", "9x40x48", "3x40x33_nonuniform")


def _create(geo, tables):
    co = mesh._grid_array([t.astype(np.float64) for t in tables])
    return np.asarray(geo.create(co), dtype=np.float32)


def _check_geometry(geo, tables, level=0.0):
    field = _create(geo, tables)
    mask = R.inside(field, level).reshape([t.size for t in tables])
    total = 0
    for connectivity, region in (("faces", "inside"), ("full", "outside"), ("full", "inside")):
        got = topology.label(geo, tables, level=level, connectivity=connectivity, region=region)
        by_field = topology.label(field, tables, level=level, connectivity=connectivity, region=region)
        np.testing.assert_array_equal(got.labels_host(), by_field.labels_host())
        _same_components(got, R.label(mask if region == "inside" else ~mask, connectivity), (connectivity, region))
        total += got.count
    assert topology.cell_counts(geo, tables, level) == R.cell_counts(mask)
    return total


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_geometry_path_equals_field_path(engine, scene):
    total = 0
    for key in GEOMETRY_GRIDS:
        total += _check_geometry(SCENES[scene](), GRIDS[key])
    assert total > 0


def test_sphere_on_2d_grids(engine):
    for key in ("2x2", "130x130", "64x200"):
        assert _check_geometry(ns.Circle(0.6), GRIDS[key]) > 0


def test_many_components_in_chain_mode(engine):
    geo = workloads.sphere_union(ns, count=64, radius=0.12)
    c = topology.label(geo, GRIDS["9x40x48"])
    assert c.count > 10 and c.sizes.sum() == np.count_nonzero(c.labels_host() >= 0)
    k = c.largest()
    assert c.sizes[k] == c.sizes.max() and k == int(np.flatnonzero(c.sizes == c.sizes.max())[0])
    lo, hi = c.box(k)
    assert np.all(lo <= hi) and lo.shape == (3,)
    for a in range(3):
        assert lo[a] == float(GRIDS["9x40x48"][a][c.lower[k, a]]) and hi[a] == float(GRIDS["9x40x48"][a][c.upper[k, a]])


@pytest.mark.parametrize("mode", [_engine.MODE_INTERPRET, _engine.MODE_SPECIALIZED])
def test_modes(engine, mode):
    geo, tables = workloads.cfg2_tree(ns), GRIDS["4x33x40"]
    want = topology.label(geo, tables, connectivity="full")
    old = config.mode
    config.mode = mode
    try:
        got = topology.label(geo, tables, connectivity="full")
        cells = topology.cell_counts(geo, tables)
    finally:
        config.mode = old
    np.testing.assert_array_equal(got.labels_host(), want.labels_host())
    assert cells == topology.cell_counts(geo, tables) and got.count == want.count > 0


def test_staged_tree_goes_through_a_resident_field(engine):
    co, res = ns.generate_grid((2, 2, 2), (25, 21, 41))
    shape = tuple(a.size for a in co.grid_axes)

    def tree():
        s = ns.Sphere(0.6)
        s.conv_averaging((3, 3, 3), 1, res)
        return s
    field = np.asarray(tree().create(co), dtype=np.float32)
    got = topology.label(tree(), co)
    _same_components(got, R.label(R.inside(field).reshape(shape), "faces"), "staged")
    assert got.count == 1 and not got.border[0]
    by_size = topology.from_geometry(tree(), (2, 2, 2), (25, 21, 41))
    np.testing.assert_array_equal(by_size.labels_host(), got.labels_host())


@pytest.mark.parametrize("name", sorted(S.ANALYTIC))
def test_betti_of_analytic_shapes(engine, name):
    geo, size, resolution, want = S.geometry(name, ns)
    co = ns.generate_grid(size, resolution)[0]
    t = topology.betti(geo, co)
    got = (t.components, t.tunnels, t.cavities)
    assert got[:len(want)] == want and got[len(want):] == (0,) * (3 - len(want)), (name, got)
    mask = R.inside(np.asarray(geo.create(co), dtype=np.float32)).reshape([a.size for a in co.grid_axes[:len(size)]])
    assert got + (t.euler,) == R.betti(mask)
    c = topology.from_geometry(S.geometry(name, ns)[0], size, resolution)
    assert c.count == want[0] and not c.border.any()
    np.testing.assert_array_equal(c.labels_host(), R.label(mask, "faces").labels)


# ---- determinism and sources ------------------------------------------------------------------------------------------------
def test_deterministic_and_labels_false(engine):
    tables = GRIDS["9x40x48"]
    field = _field(patterns("9x40x48")["noise_0.31"])
    a = topology.label(field, tables, connectivity="full")
    b = topology.label(field, tables, connectivity="full")
    c = topology.label(field, tables, connectivity="full", labels=False)
    np.testing.assert_array_equal(a.labels_host(), b.labels_host())
    for name in ("first", "sizes", "lower", "upper", "border"):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name))
        np.testing.assert_array_equal(getattr(a, name), getattr(c, name))
    assert c.labels is None and c.count == a.count
    with pytest.raises(ValueError, match="dropped"):
        c.labels_host()
    a.free()
    with pytest.raises(ValueError, match="dropped"):
        a.field()


def test_device_field_and_host_array_agree(engine):
    tables = GRIDS["64x200"]
    field = _field(patterns("64x200")["noise_0.59"])
    dev = _engine.DeviceField.from_host(field, config.device)
    a, b = topology.label(dev, tables), topology.label(field, tables)
    np.testing.assert_array_equal(a.labels_host(), b.labels_host())
    np.testing.assert_array_equal(dev.numpy(), field.ravel())                  # the source is left unchanged
    assert topology.cell_counts(dev, tables) == topology.cell_counts(field, tables)
    tagged = ns.generate_grid((2, 2), (65, 201))[0]            # (a generate_grid array stands for its axis tables)
    field = _field(np.random.default_rng(3).random((65, 201)) < 0.5)
    by_tables = topology.label(field, [np.asarray(t) for t in tagged.grid_axes[:2]])
    assert by_tables.shape == (65, 201) and by_tables.count > 1
    np.testing.assert_array_equal(topology.label(field, tagged).labels_host(), by_tables.labels_host())


# ---- label fields -------------------------------------------------------------------------------------------------------------
def test_field_of_the_largest_component_and_its_redistance(engine):
    tables = GRIDS["9x40x48"]
    geo = workloads.sphere_union(ns, count=64, radius=0.12)
    c = topology.label(geo, tables)
    want = R.label(R.inside(_create(geo, tables)).reshape(9, 40, 48), "faces")
    assert c.count == want.count > 1
    k = c.largest()
    body = c.field(keep=[k])
    try:
        assert isinstance(body, _engine.DeviceField)
        np.testing.assert_array_equal(body.numpy().reshape(9, 40, 48), np.where(want.labels == k, np.float32(-1), np.float32(1)))
        dist = redistance.redistance(body, tables)
        assert np.array_equal(dist.reshape(9, 40, 48) <= 0, want.labels == k)      # its zero set encloses that component only
        assert topology.label(dist, tables).count == 1
    finally:
        body.free()
    everything = c.field()
    np.testing.assert_array_equal(everything.numpy().reshape(9, 40, 48) < 0, want.labels >= 0)
    everything.free()
    some = np.zeros(c.count, dtype=bool)
    some[::2] = True
    half = c.field(keep=some, inside=2.5, outside=-4.0)
    np.testing.assert_array_equal(half.numpy().reshape(9, 40, 48),
                                  np.where((want.labels >= 0) & (want.labels % 2 == 0), np.float32(2.5), np.float32(-4.0)))
    half.free()
    outside = topology.label(geo, tables, region="outside", connectivity="full")
    np.testing.assert_array_equal(outside.field().numpy().reshape(9, 40, 48) < 0, want.labels < 0)
    with pytest.raises(ValueError, match="ids are"):
        c.field(keep=[c.count])


def test_too_many_points_are_refused_by_argument(engine):
    big = np.arange(1291, dtype=np.float32)
    with pytest.raises(ValueError, match=r"2\^31 - 1 points"):
        topology.label(ns.Sphere(0.5), (big, big, big))
    assert engine.lib().sdfk_label_scratch(1291, 1291, 1291) > 0       # (a size, not an allocation)
    count = _engine._i64(0)
    with _engine.DeviceBuffer(512, what="refusal") as tiny:            # (the grid is refused before the scratch is looked at)
        rc = engine.lib().sdfk_label_bits(1291, 1291, 1291, 0, 0, tiny.at(), _engine.ctypes.byref(count), tiny.at(), None, None)
    assert rc == -1 and "2^31 - 1" in engine.last_error()
