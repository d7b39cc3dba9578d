"""Component moments on the GPU (aegolius_amd.topology: Components.moments, label(..., moments=True), cavities; kernel:
sdfk_topo_moments_kernel in csrc/sdfk_topology.inc) against the numpy reference (tests/component_moments_reference.py).
The sums are integers and every comparison of them is exact equality, in dtype, shape and every entry; only the closed
forms of boxes (1e-12 relative) and the sphere's volume (a derived bound) are floating-point statements."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import aegolius_amd.cores as ns  # noqa: E402
import component_moments_reference as CM  # noqa: E402
import topology_reference as R  # noqa: E402
import topology_shapes as S  # noqa: E402
from test_gpu_topology import GRIDS, _field, patterns  # noqa: E402
from aegolius_amd import _engine, moments, topology  # noqa: E402
from aegolius_amd._eval import config  # noqa: E402

pytestmark = pytest.mark.gpu

CONNECTIVITY = ("faces", "full")
REGION = ("inside", "outside")


def _same_sums(got, want, what):
    assert got.dtype == want.dtype == np.uint64 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(got, want, err_msg=str(what))


# ---- 1. the grids and patterns of the labelling tests -------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(GRIDS))
def test_patterns_equal_the_reference(engine, key):
    tables = GRIDS[key]
    width = 10 if len(tables) == 3 else 6
    components = 0
    for name, mask in patterns(key).items():
        dev = _engine.DeviceField.from_host(_field(mask), config.device)
        try:
            for connectivity in CONNECTIVITY:
                for region in REGION:
                    what = (key, name, connectivity, region)
                    want = R.label(mask if region == "inside" else ~mask, connectivity)
                    got = topology.label(dev, tables, connectivity=connectivity, region=region)
                    m = got.moments()
                    assert m.count == got.count == want.count and m.shape == mask.shape and m.sums.shape == (want.count, width), what
                    _same_sums(m.sums, CM.sums(want.labels, want.count), what)
                    assert got.moments() is m                               # made once
                    got.free()
                    components += want.count
        finally:
            dev.free()
    assert components > 0


# ---- 2. carries ------------------------------------------------------------------------------------------------------------------
def test_sums_beyond_32_bits(engine):
    """400 x 400, all inside: the sum of i^2 is about 8.5e9 > 2^32."""
    tables = (np.linspace(-1, 1, 400), np.linspace(-1, 1, 400))
    got = topology.label(np.full(400 * 400, -1.0, dtype=np.float32), tables)
    want = CM.sums(np.zeros((400, 400), dtype=np.int32), 1)
    assert int(want[0, 3]) == 400 * sum(i * i for i in range(400)) > 2 ** 32
    _same_sums(got.moments().sums, want, "400x400")


@functools.lru_cache(maxsize=None)
def _long_rows(thirds):
    """2 x 1,000,000: (field, labels by the definition). All inside: one component. Every third column outside: the
    columns 3 m and 3 m + 1 of both rows are component m (its first point is 3 m), the last column is one of its own."""
    col = np.arange(1_000_000)
    inside = np.broadcast_to(col % 3 != 2 if thirds else col >= 0, (2, 1_000_000))
    labels = np.where(inside, col // 3 if thirds else 0, -1).astype(np.int32)
    return _field(inside), labels


@pytest.mark.parametrize("thirds", [False, True])
def test_squares_of_columns_beyond_32_bits(engine, thirds):
    """col^2 > 2^32 inside the closed forms; n (d - 1)^2 = 2e18 is below the wrap bound."""
    tables = (np.linspace(0, 1, 2), np.linspace(-1, 1, 1_000_000))
    assert not topology.sums_can_wrap((2, 1_000_000)) and 999_999 ** 2 > 2 ** 32
    field, labels = _long_rows(thirds)
    count = int(labels.max()) + 1
    assert count == (333_334 if thirds else 1)
    got = topology.label(field, tables)
    np.testing.assert_array_equal(got.labels_host(), labels)
    _same_sums(got.moments().sums, CM.sums(labels, count), "2x1000000")


# ---- 3. geometries -----------------------------------------------------------------------------------------------------------------
# every table has a step of at least 0.25, so a face midway between two grid points is 0.125 from both: the inside points
# at level 0.05 are those inside the box, and the solid of cells IS the box
BOX_GRIDS = {
    "33x33x33": tuple(np.linspace(-4, 4, 33) for _ in range(3)),
    "5x9x33": (np.linspace(-1, 1, 5), np.linspace(-1, 1, 9), np.linspace(-4, 4, 33)),
}
BOX_BLOCKS = {                                                  # per box the index range per axis, both ends included
    "33x33x33": (((3, 9), (4, 20), (5, 8)), ((14, 29), (10, 12), (17, 30))),
    "5x9x33": (((1, 2), (1, 3), (2, 9)), ((1, 3), (5, 7), (14, 29))),
}


def _box(tables, block):
    """The box whose faces lie half a step outside the block's end points -> (geometry, lower corner, upper corner)."""
    h = [(t[-1] - t[0]) / (t.size - 1) for t in tables]
    lo = np.array([t[a] - s / 2 for t, (a, _b), s in zip(tables, block, h)])
    hi = np.array([t[b] + s / 2 for t, (_a, b), s in zip(tables, block, h)])
    geo = ns.Box(*(hi - lo))
    geo.move(tuple((lo + hi) / 2))
    return geo, lo, hi


@pytest.mark.parametrize("key", sorted(BOX_GRIDS))
def test_two_boxes_have_their_own_mass_properties(engine, key):
    tables, blocks, level, rho = BOX_GRIDS[key], BOX_BLOCKS[key], 0.05, 2700.0
    union = ns.CombineGeometry("UNION").combine(_box(tables, blocks[0])[0], _box(tables, blocks[1])[0])
    c = topology.label(union, tables, level=level)
    m = c.moments()
    assert c.count == m.count == 2
    for k, block in enumerate(blocks):                         # (the first box holds the smaller first point)
        geo, lo, hi = _box(tables, block)
        alone = moments.moments(geo, tables, samples=1, level=level)
        assert m.index_moments(k) == alone.index_moments
        assert int(c.sizes[k]) == int(np.prod([b - a + 1 for a, b in block])) == m.index_moments(k)[0]
        mp = m.properties(k, rho)
        edge = hi - lo
        mass = rho * float(np.prod(edge))
        assert mp.mass == pytest.approx(mass, rel=1e-12) and mp.volume == pytest.approx(float(np.prod(edge)), rel=1e-12)
        np.testing.assert_allclose(mp.centroid, (lo + hi) / 2, rtol=1e-12, atol=1e-12 * float(edge.max()))
        second = mass * edge ** 2 / 12.0
        want = np.diag(second.sum() - second)
        np.testing.assert_allclose(np.diag(mp.inertia), np.diag(want), rtol=1e-12)
        assert np.abs(mp.inertia - want).max() <= 1e-12 * np.diag(want).max()
        np.testing.assert_allclose(m.volumes[k], float(np.prod(edge)), rtol=1e-12)
        np.testing.assert_allclose(m.centroids[k], (lo + hi) / 2, rtol=1e-12, atol=1e-12 * float(edge.max()))
    both = moments.moments(ns.CombineGeometry("UNION").combine(_box(tables, blocks[0])[0], _box(tables, blocks[1])[0]),
                           tables, samples=1, level=level)
    assert topology.index_moments(m.total()) == both.index_moments == m.total_properties().index_moments
    by_size = topology.from_geometry(ns.Sphere(0.5), (2, 2, 2), (9, 17, 33), moments=True, labels=False)
    assert by_size.labels is None and by_size.moments().count == by_size.count == 1
    assert by_size.moments().index_moments(0) == moments.from_geometry(ns.Sphere(0.5), (2, 2, 2), (9, 17, 33), samples=1).index_moments


# ---- 4. cavities -------------------------------------------------------------------------------------------------------------------
def test_cavities_of_a_hollow_sphere(engine):
    geo, size, resolution, _want = S.geometry("hollow_sphere", ns)
    co = ns.generate_grid(size, resolution)[0]
    h, r = 2.0 / 32, 0.4                                       # the shell is |r - 0.55| <= 0.15: the void is the ball r < 0.4
    v = topology.cavities(geo, co)
    assert isinstance(v, topology.ComponentMoments) and v.count == 1 and v.sums.shape == (1, 10)
    assert float(np.linalg.norm(v.centroids[0])) <= h
    # cells that can straddle the surface lie within half a cell diagonal, sqrt(3) h / 2, of it on either side
    assert abs(v.volumes[0] - 4.0 / 3.0 * np.pi * r ** 3) <= 4.0 * np.pi * r * r * np.sqrt(3.0) * h
    geo, size, resolution, _want = S.geometry("two_spheres", ns)
    none = topology.cavities(geo, ns.generate_grid(size, resolution)[0])
    assert none.count == 0 and none.sums.shape == (0, 10) and none.volumes.shape == (0,) and none.centroids.shape == (0, 3)


# ---- 5. plumbing -------------------------------------------------------------------------------------------------------------------
def test_deterministic_and_moments_without_labels(engine):
    tables = GRIDS["9x40x48"]
    field = _field(patterns("9x40x48")["noise_0.31"])
    a = topology.label(field, tables)
    b = topology.label(field, tables)
    assert a.moments().sums.tobytes() == b.moments().sums.tobytes() and a.count > 10
    c = topology.label(field, tables, labels=False, moments=True)
    assert c.labels is None and c.moments().sums.tobytes() == a.moments().sums.tobytes()
    with pytest.raises(ValueError, match="dropped"):
        c.labels_host()
    d = topology.label(field, tables, labels=False)
    with pytest.raises(ValueError, match="dropped"):
        d.moments()
    kept = a.moments()
    a.free()
    assert a.moments() is kept                                 # (made before the labels were freed)
    b.free()
    with pytest.raises(ValueError, match="dropped"):
        topology.Components((b.first, b.sizes, b.lower, b.upper, b.border), None, tables, "faces", "inside", 0.0, 0).moments()


def test_device_field_and_host_array_agree(engine):
    tables = GRIDS["64x200"]
    field = _field(patterns("64x200")["noise_0.59"])
    dev = _engine.DeviceField.from_host(field, config.device)
    a, b = topology.label(dev, tables, moments=True), topology.label(field, tables)
    _same_sums(a.moments().sums, b.moments().sums, "device field")
    np.testing.assert_array_equal(dev.numpy(), field.ravel())
    dev.free()


def test_sizes_and_boxes_agree_with_the_sums(engine):
    for key, name in (("9x40x48", "noise_0.2"), ("130x130", "noise_0.59"), ("3x40x33_nonuniform", "comb")):
        c = topology.label(_field(patterns(key)[name]), GRIDS[key], moments=True)
        sums = c.moments().sums
        np.testing.assert_array_equal(c.sizes, sums[:, 0].astype(np.int64))
        d = len(c.shape)
        for a in range(d):                                     # lower N <= I_a <= upper N, in integers
            first = sums[:, 1 + a].astype(object)
            assert np.all(c.lower[:, a].astype(object) * c.sizes.astype(object) <= first)
            assert np.all(first <= c.upper[:, a].astype(object) * c.sizes.astype(object))
    with pytest.raises(ValueError, match="not uniform"):
        c.moments().volumes                                    # (the non-uniform grid: sums, no world quantities)


def test_bad_labels_are_an_error_not_a_fault(engine):
    """Ids at or above `count`, and labels below -1, are left out and reported; the rows of the good ids are right."""
    shape = (5, 9, 33)
    rng = np.random.default_rng(11)
    labels = rng.integers(-1, 4, shape).astype(np.int32)
    with _engine.DeviceBuffer(labels.nbytes, config.device, "labels") as buf:
        buf.upload(labels)
        _same_sums(_engine.label_moments(buf, shape, 4), CM.sums(labels, 4), "any label array")
        with pytest.raises(_engine.SdfkError, match="neither -1 nor an id below 3"):
            _engine.label_moments(buf, shape, 3)
        bad = labels.copy()
        bad[2, 3, 4] = -7
        bad[4, 8, 32] = 2 ** 31 - 1
        buf.upload(bad)
        with pytest.raises(_engine.SdfkError, match="neither -1 nor an id below 4"):
            _engine.label_moments(buf, shape, 4)
