"""aegolius_amd.surface without a GPU: argument validation, the C entry's refusals (they precede the launch), the host
arithmetic of SurfacePoints, ownership of the device rows on a stand-in device, and the float64 reference's own
non-convergence on the four BASELINE scenes of the GPU test."""
import ctypes
import gc

import numpy as np
import pytest

import aegolius_amd.cores as ns
import project_reference as R
from aegolius_amd import autodiff, mesh, surface
from test_device_buffers_cpu import FakeDevice


def test_status_constants_and_symbols(built):
    assert (surface.CONVERGED, surface.MAXITER, surface.STALLED, surface.NONFINITE) == (0, 1, 2, 3)
    assert (R.CONVERGED, R.MAXITER, R.STALLED, R.NONFINITE) == (0, 1, 2, 3)
    lib = built.lib()
    for symbol in ("sdfk_project_points_device", "sdfk_project_points_counted_device", "sdfk_project_workgroups"):
        assert symbol in built.SIGNATURES and hasattr(lib, symbol)
    header = open(built.__file__.replace("aegolius_amd/_engine.py", "include/sdfk.h")).read()
    assert "int sdfk_project_points_device(sdfk_program* prog" in header
    assert [lib.sdfk_project_workgroups(n) for n in (-1, 0, 1, 256, 257)] == [0, 0, 1, 1, 2]
    assert hasattr(mesh.Mesh, "project") and hasattr(mesh.Contour, "project")


@pytest.mark.parametrize("kw, error, match", [
    (dict(max_iter=-1), ValueError, "max_iter"), (dict(max_iter=256), ValueError, "max_iter"),
    (dict(max_iter=2.0), TypeError, "max_iter"), (dict(max_iter=True), TypeError, "max_iter"),
    (dict(tol=-1e-6), ValueError, "tol"), (dict(tol=float("nan")), ValueError, "tol"),
    (dict(level=float("inf")), ValueError, "level"), (dict(level=float("nan")), ValueError, "level"),
    (dict(level=1e39), ValueError, "level"),
    (dict(relax=0.0), ValueError, "relax"), (dict(relax=1.5), ValueError, "relax"), (dict(relax=-0.5), ValueError, "relax"),
    (dict(relax=float("nan")), ValueError, "relax"),
])
def test_project_validates_its_arguments(built, kw, error, match):
    with pytest.raises(error, match=match):
        surface.project(ns.Sphere(0.5), np.zeros((3, 4)), **kw)


def test_unsupported_trees_are_refused_before_the_gpu(built):
    with pytest.raises(autodiff.UnsupportedOpError, match="has no dual rule"):
        surface.project(ns.Braid(1.0, 0.3, 0.1, 1.0), np.zeros((3, 4)))
    signed = ns.Circle(0.5)
    signed.signed((32, 32, 1))
    with pytest.raises(autodiff.UnsupportedOpError, match="staged"):
        surface.project(signed, np.zeros((3, 4)))


def _sphere_program(built, geometry=None):
    low, _ = autodiff._lower(geometry or ns.Sphere(0.5), shortcuts=True)
    return built.Program(low.code, low.params, low.tables, low.result_reg)


def test_c_entry_refusals_precede_the_launch(built):
    lib, vp = built.lib(), built._vp
    prog = _sphere_program(built)
    host = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(host)               # never dereferenced: every call below is refused before a launch

    def call(handle=prog.handle, co=ptr, n=4, row=4, level=0.0, tol=1e-5, max_iter=32, relax=1.0, q=ptr, qs=4, value=ptr,
             grad=ptr, gs=4, start=ptr, info=ptr):
        return lib.sdfk_project_points_device(handle, vp(co), n, row, level, tol, max_iter, relax, vp(q), qs, vp(value),
                                              vp(grad), gs, vp(start), vp(info), None)

    def refused(match, **kw):
        assert call(**kw) < 0
        assert match in built.last_error(), built.last_error()

    refused("null program", handle=None)
    for name in ("co", "q", "value", "info"):
        refused("null device pointer", **{name: None})
    refused("stride", row=3)
    refused("stride", qs=3)
    refused("stride", gs=3)
    refused("stride", n=-1)
    refused("max_iter", max_iter=-1)
    refused("max_iter", max_iter=256)
    refused("tol", tol=-1e-6)
    refused("tol", tol=float("nan"))
    refused("level", level=float("inf"))
    refused("level", level=float("nan"))
    refused("relax", relax=float("inf"))
    refused("relax", relax=0.0)
    refused("relax", relax=1.0000001)
    refused("relax", relax=-1.0)
    braid, _ = autodiff._lower(ns.Braid(1.0, 0.3, 0.1, 1.0), shortcuts=True)
    bad = built.Program(braid.code, braid.params, braid.tables, braid.result_reg)
    refused("no dual rule", handle=bad.handle)
    # no points: nothing is launched, whatever the machine; the gradient, its stride and the start are optional
    assert call(n=0, row=0, qs=0, gs=0) == 0
    assert call(n=0, row=0, qs=0, grad=None, gs=-5, start=None) == 0
    assert lib.sdfk_project_points_counted_device(prog.handle, vp(ptr), 0, 0, 0.0, 1e-5, 32, 1.0, vp(ptr), 0, vp(ptr),
                                                  vp(ptr), 0, vp(ptr), vp(ptr), None, None) < 0
    assert "counter" in built.last_error()


def test_surface_points_host_arithmetic():
    g = np.array([[3.0, 0.0, 0.0, 1e-30], [4.0, 0.0, -2.0, 0.0], [0.0, 0.0, 0.0, 0.0]], dtype=np.float32)
    p = np.array([[0.0, 1.0, 2.0, 3.0], [0.0, 1.0, 2.0, 3.0], [0.0, 1.0, 2.0, 3.0]], dtype=np.float32)
    q = p + np.array([[1.0, 0.0, 0.0, 0.0], [2.0, 0.0, 0.0, 3.0], [2.0, 0.0, 1e-3, 4.0]], dtype=np.float32)
    status = np.array([0, 2, 1, 3], dtype=np.uint8)
    sp = surface.SurfacePoints(q, np.zeros(4, np.float32), g, np.zeros(4, np.float32), np.zeros(4, np.uint8), status, p)
    n = sp.normals()
    assert n.dtype == np.float32 and n.shape == (4, 3)
    assert np.array_equal(n, np.array([[0.6, 0.8, 0.0], [0.0, 0.0, 0.0], [0.0, -1.0, 0.0], [1.0, 0.0, 0.0]], np.float32))
    d = sp.distance()
    assert d.dtype == np.float64
    want = np.sqrt(((q.astype(np.float64) - p.astype(np.float64)) ** 2).sum(axis=0))
    assert np.array_equal(d, want) and d[0] == 3.0 and d[1] == 0.0 and d[3] == 5.0
    assert np.array_equal(sp.converged, [True, False, False, False])
    assert "1 converged" in repr(sp) and "1 nonfinite" in repr(sp)
    resident_input = surface.SurfacePoints(q, None, g, None, None, status, None)
    with pytest.raises(ValueError, match="origin"):
        resident_input.distance()
    assert np.array_equal(resident_input.distance(p), want)
    with pytest.raises(ValueError, match="3 input points"):
        sp.distance(p[:, :3])


@pytest.fixture
def fake(built):
    real = built.lib()
    dev = FakeDevice(real)
    built._lib = dev
    try:
        yield dev
    finally:
        built._lib = real


def test_project_owns_and_releases_its_device_rows(built, fake):
    co = np.random.default_rng(2).uniform(-1, 1, (3, 70))
    geo = ns.Sphere(0.5)
    sp = surface.project(geo, co)
    gc.collect()
    allocations = fake.mallocs
    assert allocations == 6 and not fake.live and not fake.bad_frees     # coordinates, q, gradient, value, start, status
    assert fake.calls["sdfk_project_points_device"] == 1
    assert sp.points.shape == (3, 70) and sp.values.shape == (70,) and sp.status.dtype == np.uint8
    assert np.array_equal(sp.origin, co.astype(np.float32))
    for k in range(1, allocations + 1):
        fake.mallocs, fake.fail_malloc_at = 0, k
        with pytest.raises(built.SdfkError, match="out of device memory"):
            surface.project(geo, co)
        assert not fake.live and not fake.bad_frees, k
    fake.mallocs, fake.fail_malloc_at, fake.fail_h2d = 0, None, True
    with pytest.raises(built.SdfkError, match=r"sdfk_memcpy_h2d failed \(-5\)"):
        surface.project(geo, co)
    assert not fake.live and not fake.bad_frees
    # resident: the four float rows stay, owned by the existing types; free() releases them
    res = surface.project(geo, co, resident=True)
    assert isinstance(res.points, built.DeviceVectorField) and isinstance(res.gradients, built.DeviceVectorField)
    assert isinstance(res.values, built.DeviceField) and isinstance(res.start, built.DeviceField)
    assert len(fake.live) == 4
    again = surface.project(geo, res.points)                         # a resident result is an input: borrowed, not freed
    assert again.origin is None and len(fake.live) == 4
    res.free()
    gc.collect()
    assert not fake.live and not fake.bad_frees


def test_mesh_project_leaves_unconverged_vertices(built, fake, monkeypatch):
    verts = np.array([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6], [0.7, 0.8, 0.9]], dtype=np.float32)
    faces = np.array([[0, 1, 2]], dtype=np.int64)
    moved = (verts.T + 1.0).astype(np.float32)
    grads = np.array([[0.0, 2.0, 0.0], [0.0, 0.0, 0.0], [3.0, 0.0, 4.0]], dtype=np.float32).T

    def stand_in(geometry, co, level=0.0, **kw):
        assert np.array_equal(co, verts.T) and level == 0.25 and kw == dict(tol=1e-6)
        return surface.SurfacePoints(moved, np.zeros(3, np.float32), grads, np.zeros(3, np.float32),
                                     np.zeros(3, np.uint8), np.array([0, 1, 0], np.uint8), co)
    monkeypatch.setattr(surface, "project", stand_in)
    m = mesh.Mesh(verts.copy(), faces.copy())
    sp = m.project(ns.Sphere(0.5), level=0.25, tol=1e-6)
    assert np.array_equal(m.vertices, np.array([moved.T[0], verts[1], moved.T[2]])) and m.vertices.dtype == np.float32
    assert np.array_equal(m.faces, faces)
    assert np.array_equal(m.normals, np.array([[0, 1, 0], [0, 0, 0], [0.6, 0.0, 0.8]], np.float32))
    assert np.array_equal(m.normals, sp.normals())
    with pytest.raises(ValueError, match="resident"):
        m.project(ns.Sphere(0.5), resident=True)

    def stand_in_2d(geometry, co, level=0.0, **kw):
        assert np.array_equal(co[:2], verts.T[:2]) and np.all(co[2] == 0.0)
        return surface.SurfacePoints(moved, np.zeros(3, np.float32), grads, np.zeros(3, np.float32),
                                     np.zeros(3, np.uint8), np.array([0, 0, 2], np.uint8), co)
    monkeypatch.setattr(surface, "project", stand_in_2d)
    c = mesh.Contour(verts[:, :2].copy(), np.array([[0, 1], [1, 2]], dtype=np.int64))
    assert c.normals is None
    c.project(ns.Circle(0.4))
    assert c.vertices.shape == (3, 2) and np.array_equal(c.vertices, np.array([moved.T[0, :2], moved.T[1, :2], verts[2, :2]]))
    assert c.normals.shape == (3, 3)


@pytest.mark.parametrize("name", R.SCENES)
def test_reference_stays_within_the_cap(name):
    """The float64 iteration itself leaves out 0 (cfg 2), 0.15 % (cfg 5, MAXITER), 0.15 % (cfg 3, STALLED) and 0.42 %
    (cfg 4, MAXITER) of the 4096 points (6, 6 and 17 of them): the GPU test's cap of 1 % is more than twice the worst."""
    geo, size = R.scene(ns, name)
    out = R.project(geo, R.scene_points(size))
    status = out["status"]
    shares = [float(np.mean(status == k)) for k in range(4)]
    print(name, "converged %.4f maxiter %.4f stalled %.4f nonfinite %.4f" % tuple(shares))
    assert shares[R.NONFINITE] == 0.0
    assert 1.0 - shares[R.CONVERGED] <= R.CAP
    ok = status == R.CONVERGED
    assert np.all(np.abs(out["values"][ok]) <= float(np.float32(1e-5)))
    assert np.all(out["iterations"][ok] <= 32) and np.all(out["iterations"][status == R.MAXITER] == 32)
