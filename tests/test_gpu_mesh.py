"""Isosurface and contour extraction on the GPU (csrc/sdfk_mesh.inc) against the numpy definition in mesh_reference.py:
vertices, faces and segments bit for bit, plus geometric checks of the meshes."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import aegolius_amd.cores as ns  # noqa: E402
import mesh_reference as R  # noqa: E402
from aegolius_amd import _engine, _mctable, mesh, workloads  # noqa: E402

pytestmark = pytest.mark.gpu


def _grid(n, lo=-1.0, hi=1.0, dims=3):
    return [np.linspace(lo, hi, n)] * dims


def _mesh_field(fn, axes):
    g = np.meshgrid(*[np.asarray(a, dtype=np.float32).astype(np.float64) for a in axes], indexing="ij")
    return fn(*g).astype(np.float32).ravel()


def sphere(x, y, z, c=(0.05, -0.03, 0.02), r=0.6):
    return np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r


def torus(x, y, z, R0=0.5, r=0.25):
    return np.sqrt((np.sqrt(x ** 2 + y ** 2) - R0) ** 2 + z ** 2) - r


def _same(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    assert got[0].dtype == np.float32 and got[1].dtype == np.int64


def _iso(field, axes, level=0.0):
    m = mesh.isosurface(field, axes, level)
    return m.vertices, m.faces


def _con(field, axes, level=0.0):
    c = mesh.contour(field, axes, level)
    return c.vertices, c.segments


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_analytic_shapes_match_the_definition(engine, name):
    axes = _grid(65)
    f = _mesh_field(sphere if name == "sphere" else torus, axes)
    want = R.extract(f, axes)
    got = _iso(f, axes)
    _same(got, want)
    v, fc = got
    assert R.is_closed_oriented_manifold(fc)
    assert R.euler_characteristic(v, fc) == (2 if name == "sphere" else 0)
    # the oracle at the vertices, and face normals against its gradient
    h = 2.0 / 64
    fn = sphere if name == "sphere" else torus
    vv = v.astype(np.float64)
    assert np.abs(fn(vv[:, 0], vv[:, 1], vv[:, 2])).max() <= 0.02 * h
    t = vv[fc]
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    cen = t.mean(axis=1)
    eps = 1e-6
    grad = np.stack([(fn(*(cen + eps * np.eye(3)[k]).T) - fn(*(cen - eps * np.eye(3)[k]).T)) / (2 * eps) for k in range(3)], 1)
    area = np.linalg.norm(nrm, axis=1)
    ok = area > 1e-12                                   # degenerate triangles (vertices on a grid point) have no normal
    assert np.all(np.einsum("ij,ij->i", nrm[ok], grad[ok]) > 0)


def test_cfg2_tree_resident_and_host(engine):
    co, res = ns.generate_grid((2, 2, 2), (97, 97, 97))
    tree = workloads.cfg2_tree(ns)
    dev = tree.create_resident(co)
    try:
        f = dev.numpy()
        want = R.extract(f, co.grid_axes)
        got = _iso(dev, co)
        _same(got, want)
        _same(_iso(f, co.grid_axes), want)                 # host input, the three tables
        again = _iso(dev, co)
        assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()
        assert len(want[1]) > 1000 and R.is_closed_oriented_manifold(want[1])
    finally:
        dev.free()


def test_non_uniform_axes_of_three_lengths(engine):
    rng = np.random.default_rng(5)
    axes = [np.sort(rng.uniform(-1, 1, n)) for n in (41, 53, 37)]
    axes = [np.unique(a.astype(np.float32)) for a in axes]
    f = _mesh_field(lambda x, y, z: np.sqrt((x - 0.1) ** 2 / 0.5 + y ** 2 + (z + 0.05) ** 2 / 0.3) - 0.7, axes)
    _same(_iso(f, axes), R.extract(f, axes))


@pytest.mark.parametrize("level", [0.13, -0.21])
def test_level_other_than_zero(engine, level):
    axes = _grid(49)
    f = _mesh_field(torus, axes)
    want = R.extract(f, axes, level)
    _same(_iso(f, axes, level), want)
    assert len(want[1]) > 0


def test_every_case_once(engine):
    # one 2x2x2 block per case, blocks separated by a plane of outside points (the cells between blocks mesh too)
    nb = 16
    side = 3 * nb
    f = np.ones((3 * 16, 3 * 16, 3), dtype=np.float32)
    for c in range(256):
        bi, bj = divmod(c, nb)
        for corner in range(8):
            dx, dy, dz = _mctable.corner_offset3(corner)
            f[3 * bi + dx, 3 * bj + dy, dz] = -1.0 if c >> corner & 1 else 1.0
    axes = [np.linspace(0, 1, side), np.linspace(0, 2, side), np.array([0.0, 0.5, 1.0])]
    f[np.arange(side) % 3 == 2] = 0.5
    f[:, np.arange(side) % 3 == 2] = 0.5
    flat = f.ravel()
    want = R.extract(flat, axes)
    _same(_iso(flat, axes), want)


def test_random_field_with_ties_and_nans(engine):
    rng = np.random.default_rng(11)
    shape = (29, 33, 35)
    f = rng.choice(np.float32([-1.0, -0.25, 0.0, 0.0, 0.5, 1.0, 2.0]), size=shape)
    noise = rng.random(shape) < 0.1
    f[noise] = rng.standard_normal(int(noise.sum())).astype(np.float32)
    f[rng.random(shape) < 0.05] = np.nan
    axes = [np.linspace(-1, 1, s) for s in shape]
    want = R.extract(f.ravel(), axes)
    got = _iso(f.ravel(), axes)
    _same(got, want)
    assert not np.isnan(got[0]).any()
    cw = R.extract(f[:, :, 7].ravel(), axes[:2])
    _same(_con(f[:, :, 7].ravel(), axes[:2]), cw)


def test_all_outside(engine):
    axes = _grid(17)
    f = np.ones(17 ** 3, dtype=np.float32)
    v, fc = _iso(f, axes)
    assert v.shape == (0, 3) and fc.shape == (0, 3)
    v, s = _con(np.ones(17 * 17, np.float32), axes[:2])
    assert v.shape == (0, 2) and s.shape == (0, 2)


def test_contours(engine):
    axes = [np.linspace(-1, 1, 81), np.linspace(-1.2, 1.2, 97)]
    g = np.meshgrid(*[a.astype(np.float32).astype(np.float64) for a in axes], indexing="ij")
    rr = np.sqrt(g[0] ** 2 + g[1] ** 2)
    circle = (rr - 0.5).astype(np.float32).ravel()
    _same(_con(circle, axes), R.extract(circle, axes))
    annulus = np.maximum(rr - 0.8, 0.4 - rr).astype(np.float32).ravel()
    got = _con(annulus, axes)
    _same(got, R.extract(annulus, axes))
    loops = mesh.Contour(*got).loops()
    assert len(loops) == 2 and all(lp[0] == lp[-1] for lp in loops)
    areas = sorted(_area(got[0][lp]) for lp in loops)
    assert areas[0] < 0 < areas[1]                         # the hole clockwise, the outside boundary counter-clockwise


def _area(p):
    p = p.astype(np.float64)
    return 0.5 * float(np.sum(p[:-1, 0] * p[1:, 1] - p[1:, 0] * p[:-1, 1]))


def test_hourglass_2d(engine):
    import example_scenes
    geo = example_scenes.hourglass_parametric(ns)
    co, res = ns.generate_grid((4, 6), (201, 301))
    dev = geo.create_resident(co)
    try:
        f = dev.numpy()
        want = R.extract(f, co.grid_axes[:2])
        _same(_con(dev, co), want)
        assert len(want[1]) > 100
    finally:
        dev.free()
    c = mesh.from_geometry(geo, (4, 6), (201, 301))
    _same((c.vertices, c.segments), want)


def test_large_grid_scans_many_chunks(engine):
    """513^3: 16,435 tiles, more than four chunks of the scan."""
    co, res = ns.generate_grid((2, 2, 2), (513, 513, 513))
    dev = workloads.cfg2_tree(ns).create_resident(co)
    try:
        got = _iso(dev, co)
        f = dev.numpy()
    finally:
        dev.free()
    want = R.extract(f, co.grid_axes)
    assert len(got[0]) == len(want[0]) and len(got[1]) == len(want[1])
    _same(got, want)


def test_sphere_volume_and_normals(engine):
    m = mesh.from_geometry(ns.Sphere(0.5), (2, 2, 2), (257, 257, 257))
    vol = R.signed_volume(m.vertices, m.faces)
    assert abs(vol / (4 / 3 * np.pi * 0.125) - 1) < 5e-3
    small = mesh.from_geometry(ns.Sphere(0.5), (2, 2, 2), (65, 65, 65))
    small.compute_normals(ns.Sphere(0.5))
    v = small.vertices.astype(np.float64)
    want = v / np.linalg.norm(v, axis=1, keepdims=True)
    assert small.normals.shape == v.shape and small.normals.dtype == np.float32
    assert np.abs(small.normals - want).max() <= 1e-5


def test_device_field_size_is_checked(engine):
    dev = _engine.DeviceField.from_host(np.zeros(10, np.float32))
    try:
        with pytest.raises(ValueError):
            mesh.isosurface(dev, _grid(3))
    finally:
        dev.free()
