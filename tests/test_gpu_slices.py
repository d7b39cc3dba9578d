"""Plane stacks on the GPU (aegolius_amd.slices; kernels: csrc/sdfk_slices.inc) against the numpy reference
(tests/slices_reference.py) on the field of the framed geometry: vertices as uint32 bit patterns, segments and both offset
arrays; sections against the geometry's own create(); modes; independent layers; the device's section measures; and an
analytic sphere."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import aegolius_amd.cores as ns  # noqa: E402
import slices_reference as R  # noqa: E402
from aegolius_amd import _engine, mesh, moments, slices, workloads  # noqa: E402
from aegolius_amd._eval import config  # noqa: E402

pytestmark = pytest.mark.gpu


def _cloud():
    rng = np.random.default_rng(5)
    return ns.geom_3d.PointCloud3D(rng.uniform(-0.8, 0.8, (3, 300)))


SCENES = {
    "sphere": lambda: ns.Sphere(0.5),
    "cfg2_tree": lambda: workloads.cfg2_tree(ns),
    "cfg5_tree": lambda: workloads.cfg5_tree(ns),
    "sphere_union_64": lambda: workloads.sphere_union(ns, count=64, radius=0.12),      # chain mode, candidate lists
    "point_cloud_300": _cloud,                                                          # box-tree point cloud
}


def _oblique():
    u = np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)
    n = np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0)
    v = np.cross(n, u)
    return slices.Frame((0.1, -0.05, 0.2), u, v / np.linalg.norm(v))


FRAMES = {"axis0": lambda: slices.Frame.axis(0), "axis1": lambda: slices.Frame.axis(1), "axis2": lambda: slices.Frame.axis(2),
          "oblique": _oblique}


def _lin(lo, hi, n):
    return (np.linspace(lo, hi, n) + 0.0).astype(np.float32)   # (+ 0.0: no negative zero in a table)


def _nonuniform(n, seed):
    rng = np.random.default_rng(seed)
    a = np.unique(np.sort(rng.uniform(-1.0, 1.0, 4 * n)).astype(np.float32))
    return np.ascontiguousarray(a[::4][:n] + np.float32(0.0))


# (H, U, V): what each shape is there for is in the issue's list — one layer and one cell; words that straddle rows and
# layers; rows longer than a word; rows of exactly two words; non-uniform tables; three tiles
GRIDS = {
    "1x2x2": (_lin(0.1, 0.1, 1), _lin(-0.7, 0.6, 2), _lin(-0.6, 0.7, 2)),
    "2x2x2": (_lin(-0.2, 0.3, 2), _lin(-0.7, 0.6, 2), _lin(-0.6, 0.7, 2)),
    "3x5x7": (_lin(-0.4, 0.4, 3), _lin(-1, 1, 5), _lin(-1, 1, 7)),
    "4x33x40": (_lin(-0.6, 0.5, 4), _lin(-1, 1, 33), _lin(-0.9, 1.1, 40)),
    "5x9x64": (_lin(-0.5, 0.6, 5), _lin(-1, 1, 9), _lin(-1, 1, 64)),
    "3x40x33_nonuniform": (_nonuniform(3, 1), _nonuniform(40, 2), _nonuniform(33, 3)),
    "9x40x48": (_lin(-1, 1, 9), _lin(-1, 1, 40), _lin(-1, 1, 48)),
}


def _field(geo, frame, tables):
    """F[l, i, j]: Frame.apply(geo).create() on the grid (H, U, V), float32."""
    co = mesh._grid_array([t.astype(np.float64) for t in tables])
    return np.asarray(frame.apply(geo).create(co), dtype=np.float32).reshape([t.size for t in tables])


def _levels(F):
    near = float(F.ravel()[int(np.nanargmin(np.abs(F)))])      # a level that IS a value of F at a grid point
    return [0.0, -0.05, 0.05, near]


def _arrays(st):
    return st.vertices, st.segments, st.vertex_offsets, st.segment_offsets


def _same(got, want):
    gv, gs, gvo, gso = got
    wv, ws, wvo, wso = want
    assert gv.dtype == wv.dtype == np.float32 and gs.dtype == ws.dtype == np.int64
    assert gvo.dtype == np.int64 and gso.dtype == np.int64
    np.testing.assert_array_equal(gvo, wvo)
    np.testing.assert_array_equal(gso, wso)
    assert gv.shape == wv.shape and gs.shape == ws.shape
    np.testing.assert_array_equal(gv.view(np.uint32), wv.view(np.uint32))
    np.testing.assert_array_equal(gs, ws)


def _check(geo, frame, tables, levels=None):
    F = _field(geo, frame, tables)
    total = 0
    for lv in (levels or _levels(F)):
        got = slices.stack(geo, tables[1:], tables[0], normal=frame, level=lv)
        _same(_arrays(got), R.stack(F, tables[1:], lv))
        total += len(got.segments)
    return total


@pytest.mark.parametrize("frame", sorted(FRAMES))
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_stack_equals_the_reference_bit_for_bit(engine, scene, frame):
    geo, fr = SCENES[scene](), FRAMES[frame]()
    total = sum(_check(geo, fr, tables) for tables in GRIDS.values())
    assert total > 0


@pytest.mark.parametrize("frame", sorted(FRAMES))
@pytest.mark.parametrize("layers", [(6, 7, 8), (0, 1, 2)])
def test_empty_tiles_and_boundaries_inside_them(engine, layers, frame):
    """9 x 40 x 48 points are three tiles of 8192; a layer has 1920. A sphere inside layers 6 - 8 leaves the first tile
    without output, with the layer boundaries 1 - 4 inside it; inside layers 0 - 2 it leaves the last two tiles empty."""
    fr, tables = FRAMES[frame](), GRIDS["9x40x48"]
    geo = ns.Sphere(0.3)
    geo.move(fr.world(float(tables[0][layers[1]]), 0.05, -0.1))
    F = _field(geo, fr, tables)
    got = slices.stack(geo, tables[1:], tables[0], normal=fr)
    _same(_arrays(got), R.stack(F, tables[1:], 0.0))
    per_layer = np.diff(got.segment_offsets)
    assert np.all(per_layer[list(layers)] > 0) and per_layer.sum() == per_layer[list(layers)].sum()


@pytest.mark.parametrize("normal", [0, 1, 2])
@pytest.mark.parametrize("scene", ["sphere", "cfg2_tree", "cfg5_tree"])
def test_axis_sections_are_sections_of_create(engine, scene, normal):
    """The reference on the ORIGINAL geometry's create() on the world grid, transposed to layer-major."""
    geo = SCENES[scene]()
    for name in ("3x5x7", "4x33x40", "5x9x64"):
        H, U, V = GRIDS[name]
        world = [None] * 3
        world[normal], world[(normal + 1) % 3], world[(normal + 2) % 3] = H, U, V
        Fw = np.asarray(geo.create(mesh._grid_array([t.astype(np.float64) for t in world])), dtype=np.float32)
        F = np.transpose(Fw.reshape([t.size for t in world]), (normal, (normal + 1) % 3, (normal + 2) % 3))
        for lv in _levels(F):
            _same(_arrays(slices.stack(geo, (U, V), H, normal=normal, level=lv)), R.stack(F, (U, V), lv))


def test_axis_sections_with_the_specialised_kernels(engine):
    """MODE_AUTO starts on the interpreter kernel while the specialised one builds; here both sides wait for the build
    (row-block kernels with cull sites, brick-tiled flags)."""
    geo = workloads.cfg2_tree(ns)
    H, U, V = GRIDS["4x33x40"]
    old = config.mode
    config.mode = _engine.MODE_SPECIALIZED
    try:
        Fw = np.asarray(geo.create(mesh._grid_array([t.astype(np.float64) for t in (U, V, H)])), dtype=np.float32)
        F = np.transpose(Fw.reshape(U.size, V.size, H.size), (2, 0, 1))
        got = slices.stack(geo, (U, V), H, normal=2)
    finally:
        config.mode = old
    assert len(got.segments) > 0
    _same(_arrays(got), R.stack(F, (U, V), 0.0))
    _same(_arrays(got), _arrays(slices.stack(geo, (U, V), H, normal=2)))


@pytest.mark.parametrize("mode", [_engine.MODE_INTERPRET, _engine.MODE_NOCULL, _engine.MODE_SPECIALIZED])
def test_modes(engine, mode):
    geo, fr, tables = workloads.cfg2_tree(ns), _oblique(), GRIDS["4x33x40"]
    want = [_arrays(slices.stack(geo, tables[1:], tables[0], normal=fr, level=lv)) for lv in (0.0, 0.05)]
    old = config.mode
    config.mode = mode
    try:
        for lv, w in zip((0.0, 0.05), want):
            _same(_arrays(slices.stack(geo, tables[1:], tables[0], normal=fr, level=lv)), w)
    finally:
        config.mode = old


def test_deterministic(engine):
    geo, tables = workloads.cfg5_tree(ns), GRIDS["4x33x40"]
    a = slices.stack(geo, tables[1:], tables[0], normal=1)
    b = slices.stack(geo, tables[1:], tables[0], normal=1)
    assert len(a.segments) > 0
    for x, y in zip(_arrays(a), _arrays(b)):
        assert x.tobytes() == y.tobytes()
    ma = slices.measures(geo, tables[1:], tables[0], normal=1)
    mb = slices.measures(geo, tables[1:], tables[0], normal=1)
    for name in ("area", "perimeter", "moments", "centroid", "segments", "border"):
        assert getattr(ma, name).tobytes() == getattr(mb, name).tobytes()


@pytest.mark.parametrize("frame", ["axis2", "oblique"])
def test_layers_are_independent(engine, frame):
    geo, fr = workloads.cfg2_tree(ns), FRAMES[frame]()
    H, U, V = GRIDS["5x9x64"][0], GRIDS["4x33x40"][1], GRIDS["4x33x40"][2]
    whole = slices.stack(geo, (U, V), H, normal=fr)
    assert len(whole) == 5 and len(whole.layer(2).segments) > 0
    for l in (0, 2, 4):
        one = slices.stack(geo, (U, V), H[l:l + 1], normal=fr)
        assert one.vertex_offsets.tolist() == [0, len(one.vertices)] and one.segment_offsets.tolist() == [0, len(one.segments)]
        c, d = whole.layer(l), one.layer(0)
        np.testing.assert_array_equal(c.vertices.view(np.uint32), d.vertices.view(np.uint32))
        np.testing.assert_array_equal(c.segments, d.segments)


def _compare_measures(got, st):
    """Device measures against the reference on the downloaded stack: counts exact, float sums to the summation order."""
    want = R.measures(st.vertices, st.segments, st.vertex_offsets, st.segment_offsets, st.axes)
    np.testing.assert_array_equal(got.segments, want["segments"])
    np.testing.assert_array_equal(got.border, want["border"])
    np.testing.assert_array_equal(got.closed, want["closed"])
    np.testing.assert_array_equal(np.isnan(got.area), ~want["closed"])
    eps = 2.0 ** -53
    S = want["segments"].astype(np.float64)
    tol_t = S * eps * want["abs_t"]
    ok = want["closed"]
    d_area = np.abs(got.area[ok] - want["area"][ok])
    d_mom = np.abs(got.moments - want["moments"]).max(axis=1)
    d_per = np.abs(got.perimeter - want["perimeter"])
    print("measures: max area diff %.3e (bound %.3e), moments %.3e (%.3e), perimeter %.3e (%.3e)"
          % (d_area.max(initial=0.0), tol_t[ok].max(initial=0.0), d_mom.max(initial=0.0), tol_t.max(initial=0.0),
             d_per.max(initial=0.0), (S * eps * want["perimeter"]).max(initial=0.0)))
    assert np.all(d_area <= tol_t[ok])
    assert np.all(d_mom <= tol_t)
    assert np.all(d_per <= S * eps * want["perimeter"])
    return want


@pytest.mark.parametrize("scene, frame, grid", [("cfg2_tree", "oblique", "4x33x40"), ("cfg5_tree", "axis1", "9x40x48"),
                                                ("sphere_union_64", "axis2", "5x9x64"), ("sphere", "axis0", "1x2x2")])
def test_measures_equal_the_reference_on_the_downloaded_stack(engine, scene, frame, grid):
    geo, fr, tables = SCENES[scene](), FRAMES[frame](), GRIDS[grid]
    for lv in (0.0, 0.05):
        st = slices.stack(geo, tables[1:], tables[0], normal=fr, level=lv)
        got = slices.measures(geo, tables[1:], tables[0], normal=fr, level=lv)
        _compare_measures(got, st)
        host = st.measures()                                   # the same numbers from the downloaded arrays
        np.testing.assert_array_equal(host.border, got.border)
        np.testing.assert_allclose(host.perimeter, got.perimeter, rtol=1e-12)
        np.testing.assert_allclose(host.area, got.area, rtol=1e-9, atol=1e-12, equal_nan=True)


def test_a_solid_that_leaves_the_rectangle_is_open(engine):
    geo = ns.Sphere(0.5)
    H, U, V = _lin(-0.6, 0.6, 7), _lin(-0.3, 1.0, 27), _lin(-1, 1, 41)       # cut at a = -0.3
    st = slices.stack(geo, (U, V), H)
    got = slices.measures(geo, (U, V), H)
    want = _compare_measures(got, st)
    r = np.sqrt(np.maximum(0.25 - H.astype(np.float64) ** 2, 0.0))
    assert (r > 0.35).sum() >= 3
    for l in range(len(H)):
        if r[l] > 0.35:                                        # the disc crosses a = -0.3: an open layer
            assert not got.closed[l] and got.border[l] == 2 and np.isnan(got.area[l]) and np.all(np.isnan(got.centroid[l]))
            assert got.perimeter[l] > 0
        elif r[l] == 0.0:                                      # |h| = 0.6: no contour at all
            assert got.closed[l] and got.segments[l] == 0 and got.area[l] == 0.0
    assert np.isnan(got.volume()) and want["border"].sum() > 0
    loops = st.layer(3).loops()
    assert len(loops) == 1 and loops[0][0] != loops[0][-1]    # one open chain


G = 1.0 / 64.0


@pytest.mark.parametrize("frame", ["axis2", "oblique_centre"])
def test_sphere_sections_against_the_circle(engine, frame):
    """Sphere of radius 0.5 at the origin, in-plane spacing g = 1/64, |h| <= 0.25: the section is a circle of radius
    r = sqrt(0.25 - h^2) >= 0.433, every layer closed and one loop, and |area - pi r^2| <= 3 g^2.

    Where the 3 comes from. The contour is a polygon whose vertices lie on grid edges near the circle.
      * Chord deficit. A polygon inscribed in the circle with chords c_i misses sum c_i^3 / (12 r) of its area (to leading
        order); a chord lies inside one cell, c_i <= sqrt(2) g, and sum c_i <= 2 pi r, so the deficit is at most
        2 g^2 / (12 r) * 2 pi r = pi g^2 / 3 = 1.05 g^2.
      * Vertex displacement. A vertex is the zero of the linear interpolant of f = |p| - 0.5 along a grid edge that
        crosses the surface, so every point of the edge has |p| >= 0.5 - g and |f''| <= 1 / (0.5 - g) along it; the
        interpolant is off by at most g^2 / (8 (0.5 - g)) = 0.26 g^2. In the plane |grad f| = r / 0.5 >= 0.85, so the
        contour moves along its normal by at most 0.26 g^2 / 0.85, and over a perimeter 2 pi r <= pi the area changes by
        at most 0.96 g^2.
    Both shrink the section (f is convex along an edge), so they add: 2.01 g^2; the rest of the 3 is margin for the
    second-order terms of both estimates (relative size g / r = 0.04) and for float32 (1e-7 pi / 0.85, nothing)."""
    fr = slices.Frame.axis(2) if frame == "axis2" else slices.Frame((0.0, 0.0, 0.0), _oblique().u, _oblique().v)
    geo = ns.Sphere(0.5)
    U = V = _lin(-40 * G, 40 * G, 81)
    H = _lin(-0.25, 0.25, 9)
    st = slices.stack(geo, (U, V), H, normal=fr)
    got = slices.measures(geo, (U, V), H, normal=fr)
    assert got.closed.all()
    err = np.abs(got.area - np.pi * (0.25 - H.astype(np.float64) ** 2))
    print("sphere sections (%s): max |area - pi r^2| = %.3f g^2; bound 3 g^2" % (frame, err.max() / G ** 2))
    for l in range(len(H)):
        loops = st.layer(l).loops()
        assert len(loops) == 1 and loops[0][0] == loops[0][-1]
    assert np.all(err <= 3 * G * G)
    # centroid: a first moment is off by at most the area error times the largest |a| on the contour, 3 g^2 * 0.5; divided
    # by the area (>= pi * 0.1875 = 0.589) that is 2.6 g^2
    np.testing.assert_allclose(got.centroid, 0.0, atol=3 * G * G)
    # a vertex is a zero of the interpolant, so its own |f| is the interpolation error (float32 coordinates: 1e-6 is ample)
    w = st.world_vertices()
    assert np.abs(np.linalg.norm(w, axis=1) - 0.5).max() <= G * G / (8 * (0.5 - G)) + 1e-6


def test_sphere_volume_against_the_moments(engine):
    """volume() of the z-stack of generate_grid((1.25,) * 3, (81,) * 3) (spacing g = 1/64 along every axis, heights over
    |h| <= 0.625, so over the whole sphere) against moments.from_geometry on the same grid with 8 sub-samples per axis.

    Bound on |volume() - pi / 6|. Per layer, as in test_sphere_sections_against_the_circle with the slope 2 r instead of
    0.85: the displacement term is (g^2 / (8 (0.5 - g))) / (2 r) * 2 pi r = 0.81 g^2 whatever r, the chord term
    pi g^2 / 3, 1.86 g^2 together; 3 g^2 with the same margin (the first layer off a pole has r = 8 g already; the pole
    layers and those beyond have area 0 on both sides). The trapezoid weights sum to the height 1, so the layers add at
    most 3 g^2. The trapezoid rule itself, on the concave parabola A(h) = pi (0.25 - h^2) with A'' = -2 pi over a length
    of 1: g^2 * 2 pi / 12 = pi g^2 / 6. Together (3 + pi / 6) g^2 = 3.52 g^2.
    Bound on |moments volume - pi / 6|: it counts sub-cells of edge s = g / 8 whose centre is inside. A sub-cell that is
    all inside or all outside is counted right; one that the surface crosses has its centre within half a diagonal,
    sqrt(3) s / 2, of the surface, and is counted wrong by at most half its volume up to curvature (the sphere is convex
    and its radius is 256 s). The shell of that half-thickness has the volume pi sqrt(3) s (surface area pi), half of it
    is 2.72 s = 0.34 g = 21.8 g^2.
    The test allows the sum, 25.3 g^2 = 6.2e-3 (1.2 % of the volume): the moments' own bound dominates it."""
    geo = ns.Sphere(0.5)
    st = slices.from_geometry(geo, (1.25, 1.25, 1.25), (81, 81, 81), normal=2)
    np.testing.assert_allclose(np.diff(st.heights.astype(np.float64)), G, rtol=1e-6)
    m = st.measures()
    assert m.closed.all() and len(m) == 81
    mp = moments.from_geometry(geo, (1.25, 1.25, 1.25), (81, 81, 81), samples=8)
    v_stack, v_mom, v_true = m.volume(), mp.volume, np.pi / 6
    print("sphere volume: stack %.9f (%.3f g^2 off pi/6), moments %.9f (%.3f g^2 off), difference %.3f g^2; bound 25.3 g^2"
          % (v_stack, abs(v_stack - v_true) / G ** 2, v_mom, abs(v_mom - v_true) / G ** 2, abs(v_stack - v_mom) / G ** 2))
    assert abs(v_stack - v_true) <= (3 + np.pi / 6) * G * G
    assert abs(v_stack - v_mom) <= (3 + np.pi / 6 + 0.5 * np.pi * np.sqrt(3.0) / 8 * 64) * G * G
    dev = slices.measures(geo, (st.axes[0], st.axes[1]), st.heights, normal=2)
    np.testing.assert_allclose(dev.volume(), v_stack, rtol=1e-12)


def test_timings(engine):
    t = {}
    tables = GRIDS["4x33x40"]
    slices.stack(workloads.cfg2_tree(ns), tables[1:], tables[0], timings=t)
    assert set(t) == {"count", "emit", "copy"}
    slices.measures(workloads.cfg2_tree(ns), tables[1:], tables[0], timings=t)
    assert set(t) == {"count", "emit", "copy", "measure"}
    assert all(np.isfinite(v) and v >= 0 for v in t.values())
