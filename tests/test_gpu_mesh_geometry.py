"""Meshing a geometry without a field (aegolius_amd.mesh, geometry path; kernels: csrc/sdfk_mesh.inc) against the field
path on the same grid: vertices as uint32 bit patterns, faces, dtypes. The field path's field comes from the axis tables
(Program.eval_grid into a DeviceField, what create_resident does with a generate_grid array)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import aegolius_amd.cores as ns  # noqa: E402
import example_scenes  # noqa: E402
import mesh_reference as R  # noqa: E402
import scenes  # noqa: E402
from aegolius_amd import _engine, mesh, workloads  # noqa: E402
from aegolius_amd._eval import config, program_for  # noqa: E402
from aegolius_amd._lower import lower_geometry  # noqa: E402

pytestmark = pytest.mark.gpu


def _cloud():
    rng = np.random.default_rng(5)
    return ns.geom_3d.PointCloud3D(rng.uniform(-0.8, 0.8, (3, 300)))


SCENES = {
    "cfg1_sphere": lambda: workloads.cfg1_sphere(ns),
    "cfg2_tree": lambda: workloads.cfg2_tree(ns),
    "cfg3_chain": lambda: workloads.cfg3_chain(ns),
    "cfg5_tree": lambda: workloads.cfg5_tree(ns),
    "sphere_union_1000": lambda: workloads.sphere_union(ns, count=1000),
    "point_cloud_300": _cloud,
}


def _nonuniform():
    rng = np.random.default_rng(11)
    out = []
    for n in (23, 41, 36):
        a = np.unique(np.sort(rng.uniform(-1.0, 1.0, n)).astype(np.float32))
        out.append(a.astype(np.float64))
    return out


GRIDS = {
    "2^3": [np.linspace(-1, 1, 2)] * 3,
    "3x5x7": [np.linspace(-1, 1, 3), np.linspace(-1, 1, 5), np.linspace(-1, 1, 7)],
    "33x31x64": [np.linspace(-1, 1, 33), np.linspace(-0.9, 1.1, 31), np.linspace(-1, 1, 64)],
    "7x50x40": [np.linspace(-1, 1, 7), np.linspace(-1, 1, 50), np.linspace(-1, 1, 40)],
    "5x5x333": [np.linspace(-1, 1, 5), np.linspace(-1, 1, 5), np.linspace(-1, 1, 333)],
    "97^3": [np.linspace(-1, 1, 97)] * 3,
    "nonuniform": _nonuniform(),
}


def _field(geo, axes):
    """The field of geo on the grid of the axis tables, resident (as _eval._run_resident evaluates a tagged grid)."""
    ax = [np.asarray(a, dtype=np.float64) for a in axes] + [np.zeros(1)] * (3 - len(axes))
    n = int(np.prod([a.size for a in ax]))
    field = _engine.DeviceField(n, config.device)
    program_for(lower_geometry(geo)).eval_grid(ax, 0, n, field.ptr, mode=config.mode)
    _engine.check(_engine.lib().sdfk_sync(None), "sdfk_sync")
    return field


def _same(got, want):
    gv, gf = got
    wv, wf = want
    assert gv.dtype == wv.dtype == np.float32 and gf.dtype == wf.dtype == np.int64
    assert gv.shape == wv.shape and gf.shape == wf.shape
    np.testing.assert_array_equal(gv.view(np.uint32), wv.view(np.uint32))
    np.testing.assert_array_equal(gf, wf)


def _iso(obj, axes, level):
    m = mesh.isosurface(obj, axes, level)
    return m.vertices, m.faces


def _con(obj, axes, level):
    c = mesh.contour(obj, axes, level)
    return c.vertices, c.segments


def _levels(f):
    lo, hi = float(np.nanmin(f)), float(np.nanmax(f))
    return [0.0, -0.05, 0.05, lo - 1.0, hi + 1.0]


def _check_scene(geo, axes, levels=None):
    dev = _field(geo, axes)
    try:
        f = dev.numpy()
        for lv in (levels or _levels(f)):
            want = _iso(dev, axes, lv)
            got = _iso(geo, axes, lv)
            _same(got, want)
            if lv < float(np.nanmin(f)) or lv > float(np.nanmax(f)):
                assert got[0].shape == (0, 3) and got[1].shape == (0, 3)
    finally:
        dev.free()


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_geometry_path_equals_field_path(engine, scene):
    geo = SCENES[scene]()
    for name, axes in GRIDS.items():
        _check_scene(geo, axes)


def test_cfg2_on_257_cubed(engine):
    _check_scene(workloads.cfg2_tree(ns), [np.linspace(-1, 1, 257)] * 3, levels=[0.0, -0.03, 0.04])


@pytest.mark.parametrize("mode", [_engine.MODE_INTERPRET, _engine.MODE_NOCULL])
def test_modes(engine, mode):
    old = config.mode
    config.mode = mode
    try:
        _check_scene(workloads.cfg2_tree(ns), GRIDS["97^3"], levels=[0.0, -0.05, 0.05])
    finally:
        config.mode = old


def test_contour_cfg4_scene2d(engine):
    geo = workloads.cfg4_scene2d(ns)
    axes = [np.linspace(-1, 1, 1025)] * 2
    dev = _field(geo, axes)
    try:
        for lv in (0.0, -0.02, 0.03):
            _same(_con(geo, axes, lv), _con(dev, axes, lv))
    finally:
        dev.free()


def test_contour_hourglass(engine):
    geo = example_scenes.hourglass_parametric(ns)
    co, _ = ns.generate_grid((4, 6), (201, 301))
    dev = geo.create_resident(co)
    try:
        for lv in (0.0, 0.1):
            _same(_con(geo, co, lv), _con(dev, co, lv))
    finally:
        dev.free()


def test_from_geometry_equals_the_explicit_composition(engine, monkeypatch):
    geo = workloads.cfg2_tree(ns)
    co, _ = ns.generate_grid((2, 2, 2), (65, 65, 65))
    dev = geo.create_resident(co)
    try:
        want = _iso(dev, co, 0.0)
    finally:
        dev.free()
    m = mesh.from_geometry(geo, (2, 2, 2), (65, 65, 65))
    _same((m.vertices, m.faces), want)
    geo2 = example_scenes.hourglass_parametric(ns)
    co2, _ = ns.generate_grid((4, 6), (201, 301))
    dev = geo2.create_resident(co2)
    try:
        want2 = _con(dev, co2, 0.0)
    finally:
        dev.free()

    def no_grid(*args, **kwargs):
        raise AssertionError("generate_grid was called")
    monkeypatch.setattr(ns, "generate_grid", no_grid)
    m = mesh.from_geometry(geo, (2, 2, 2), (65, 65, 65))
    _same((m.vertices, m.faces), want)
    c = mesh.from_geometry(geo2, (4, 6), (201, 301))
    _same((c.vertices, c.segments), want2)


def test_staged_tree_falls_back_to_the_field(engine):
    name = "grid_conv_sphere_3x3x3"
    build, key = scenes.GRID_SCENES[name]
    size, res = scenes.GRIDS[key]
    co, _ = ns.generate_grid(size, res)
    dev = build(ns, res).create_resident(co)
    try:
        want = _iso(dev, co, 0.0)
    finally:
        dev.free()
    got = _iso(build(ns, res), co, 0.0)
    assert len(got[1]) > 0
    _same(got, want)


def test_deterministic(engine):
    geo = workloads.cfg2_tree(ns)
    axes = GRIDS["97^3"]
    a, b = _iso(geo, axes, 0.0), _iso(geo, axes, 0.0)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_timings(engine):
    t = {}
    mesh.isosurface(workloads.cfg2_tree(ns), GRIDS["97^3"], 0.0, timings=t)
    assert set(t) == {"count", "emit", "copy"}
    assert all(np.isfinite(v) and v >= 0 for v in t.values())


def test_cfg2_at_2049_cubed(engine):
    geo = workloads.cfg2_tree(ns)
    axes = [np.linspace(-1, 1, 2049)] * 3
    dev = _field(geo, axes)
    try:
        want = _iso(dev, axes, 0.0)
    finally:
        dev.free()
    got = _iso(geo, axes, 0.0)
    assert len(got[0]) == len(want[0]) and len(got[1]) == len(want[1])
    _same(got, want)


def test_capacity_at_4097_cubed(engine):
    """The field path cannot run here (a 275 GB field); two disjoint spheres: cull sites, so brick-tiled flags."""
    a, b = ns.Sphere(0.35), ns.Sphere(0.3)
    a.move((-0.45, 0.0, 0.05))
    b.move((0.5, 0.1, -0.1))
    geo = ns.CombineGeometry("UNION").combine(a, b)
    axes = [np.linspace(-1, 1, 4097)] * 3
    assert _engine.lib().sdfk_eval_grid_isosurface_scratch(4097, 4097, 4097) <= 4097 ** 3
    m = mesh.isosurface(geo, axes, 0.0)
    V, F = len(m.vertices), len(m.faces)
    assert F > 0 and V - F // 2 == 4 and F % 2 == 0
    h = 2.0 / 4096
    v = m.vertices.astype(np.float64)
    da = np.abs(np.linalg.norm(v - (-0.45, 0.0, 0.05), axis=1) - 0.35)
    db = np.abs(np.linalg.norm(v - (0.5, 0.1, -0.1), axis=1) - 0.3)
    assert float(np.minimum(da, db).max()) <= 0.02 * h
    assert np.bincount(m.faces.ravel(), minlength=V).min() > 0


def test_small_analytic_mesh_against_the_definition(engine):
    geo = ns.Sphere(0.6)
    axes = GRIDS["33x31x64"]
    dev = _field(geo, axes)
    try:
        f = dev.numpy()
    finally:
        dev.free()
    _same(_iso(geo, axes, 0.0), R.extract(f, [np.asarray(a, dtype=np.float32) for a in axes]))
