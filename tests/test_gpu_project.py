"""aegolius_amd.surface.project on the GPU (kernel: csrc/sdfk_project.inc): one step against the float32 formula on the
dual kernel's own value and gradient, chaining, create()'s values, the analytic sphere, Lipschitz soundness, the cap on
non-convergence against the float64 reference (tests/project_reference.py), levels, sizes and the wave vote, resident
rows, refusals, and the mesh / contour consumers."""
import ctypes
import functools
import gc

import numpy as np
import pytest

import aegolius_amd.cores as ns
import autodiff_scenes
import project_reference as R
from aegolius_amd import autodiff, mesh, surface, workloads
from aegolius_amd._lower import lower_geometry

pytestmark = pytest.mark.gpu

TOL = float(np.float32(1e-5))
OP_SCENES = sorted(autodiff_scenes.OP_GEOMETRIES)
FIELDS = ("points", "values", "gradients", "start", "iterations", "status")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b, what=""):
    """Two SurfacePoints (or dicts of their fields) are equal bit for bit."""
    for name in FIELDS:
        x, y = (a[name] if isinstance(a, dict) else getattr(a, name)), (b[name] if isinstance(b, dict) else getattr(b, name))
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), "%s: %s differs" % (what, name)


def _fields(sp, index=None):
    return {name: (getattr(sp, name) if index is None else getattr(sp, name)[..., index]) for name in FIELDS}


def _geometry(name):
    """-> (geometry, points (3, 4096) float32): a BASELINE config in its box, or an OP_GEOMETRIES entry in [-1.6, 1.6]^dim."""
    if name in workloads.BASELINE:
        geo, size = R.scene(ns, name)
        return geo, R.scene_points(size)
    make, dim, _targets, _regions = autodiff_scenes.OP_GEOMETRIES[name]
    return make(ns, *autodiff_scenes.OP_DEFAULTS), R.scene_points((3.2,) * dim)


def _create(name_or_geometry, co):
    geo = _geometry(name_or_geometry)[0] if isinstance(name_or_geometry, str) else name_or_geometry
    out = geo.create(np.asarray(co, dtype=np.float32).astype(np.float64))
    assert out.dtype == np.float32
    return out


@functools.lru_cache(maxsize=None)
def _projected(name):
    """The test-6 run of a BASELINE scene (tol 1e-5, 32 steps): shared, never modified."""
    geo, p = _geometry(name)
    sp = surface.project(geo, p, tol=1e-5, max_iter=32)
    for a in (sp.points, sp.values, sp.gradients, sp.start, sp.iterations, sp.status, p):
        a.setflags(write=False)
    return sp, p


# ---- 1. one step, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg2", "cfg5", "cfg3"] + OP_SCENES)
def test_one_step_is_the_float32_formula(engine, name):
    geo, p = _geometry(name)
    f, g = autodiff.value_and_grad_points(geo, p)
    q, st = R.step_f32(p, f, g, 0.0, TOL)
    sp = surface.project(_geometry(name)[0], p, max_iter=1)
    assert np.array_equal(_bits(sp.start), _bits(f))
    assert np.array_equal(_bits(sp.points), _bits(q))
    assert np.array_equal(sp.iterations, (st < 0).astype(np.uint8))
    stopped = st >= 0
    assert np.array_equal(sp.status[stopped], st[stopped].astype(np.uint8))
    assert np.array_equal(_bits(sp.values[stopped]), _bits(f[stopped]))
    assert np.array_equal(_bits(sp.gradients[:, stopped]), _bits(g[:, stopped]))
    # a point that stepped is judged at its new place: converged there, or out of steps (or off the field's domain)
    assert np.all(np.isin(sp.status[~stopped], (surface.CONVERGED, surface.MAXITER, surface.NONFINITE)))
    assert np.array_equal(sp.origin, p) and sp.points.dtype == np.float32 and sp.status.dtype == np.uint8


# ---- 2. chaining ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg2", "cfg5", "cfg3"])
def test_iterations_chain(engine, name):
    geo, p = _geometry(name)
    chained, steps, q = {}, np.zeros(p.shape[1], dtype=np.int64), p
    for n in range(1, 33):
        sp = surface.project(geo, q, max_iter=1)
        steps = steps + sp.iterations
        q = sp.points
        if n in (2, 5, 32):
            chained[n] = dict(_fields(sp), iterations=steps.astype(np.uint8), start=None)
    f0 = _create(name, p)
    for n, want in chained.items():
        got = surface.project(geo, p, max_iter=n)
        want["start"] = f0
        _same(_fields(got), want, "%s, %d steps" % (name, n))
    zero = surface.project(geo, p, max_iter=0)
    assert np.array_equal(_bits(zero.points), _bits(p)) and np.array_equal(_bits(zero.values), _bits(f0))
    assert np.array_equal(_bits(zero.start), _bits(f0)) and not zero.iterations.any()
    assert np.array_equal(zero.status, np.where(np.abs(f0) <= np.float32(TOL), surface.CONVERGED, surface.MAXITER))


# ---- 3. values are create()'s -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg2", "cfg5"])
def test_values_are_creates(engine, name):
    sp, p = _projected(name)
    assert np.array_equal(_bits(sp.values), _bits(_create(name, sp.points)))
    assert np.array_equal(_bits(sp.start), _bits(_create(name, p)))
    assert np.array_equal(sp.status == surface.CONVERGED, np.abs(sp.values - np.float32(0.0)) <= np.float32(TOL))
    assert np.array_equal(sp.converged, sp.status == surface.CONVERGED)


# ---- 4. sphere, analytic ----------------------------------------------------------------------------------------------------
CENTRE, RADIUS = (0.2, -0.1, 0.3), 0.5


def _moved_sphere():
    s = ns.Sphere(RADIUS)
    s.move(CENTRE)
    return s


def test_sphere_is_projected_radially(engine):
    p = R.scene_points((2.0, 2.0, 2.0))
    sp = surface.project(_moved_sphere(), p, tol=1e-5, max_iter=32)
    assert np.all(sp.status == surface.CONVERGED) and sp.iterations.max() <= 2
    c = np.asarray(CENTRE, dtype=np.float64)[:, None]
    d = p.astype(np.float64) - c
    radial = d / np.linalg.norm(d, axis=0)
    err = np.linalg.norm(sp.points.astype(np.float64) - (c + RADIUS * radial), axis=0)
    print("sphere: max |q - q*| %.3e, max steps %d" % (err.max(), sp.iterations.max()))
    assert err.max() <= 2 * TOL
    # the gradient of the distance to a sphere points away from the centre on both sides of the surface
    cosine = np.sum(sp.normals().astype(np.float64).T * radial, axis=0)
    assert cosine.min() >= 1 - 1e-6
    assert np.array_equal(sp.distance(), np.linalg.norm(sp.points.astype(np.float64) - p.astype(np.float64), axis=0))


def test_sphere_centre_stalls(engine):
    p = np.array([CENTRE, (0.9, 0.1, 0.3)], dtype=np.float32).T.copy()
    sp = surface.project(_moved_sphere(), p)
    assert sp.status[0] == surface.STALLED and sp.iterations[0] == 0 and np.array_equal(_bits(sp.points[:, 0]), _bits(p[:, 0]))
    assert sp.values[0] == np.float32(-RADIUS) and sp.start[0] == np.float32(-RADIUS)
    assert np.all(np.isfinite(sp.points)) and np.all(np.isfinite(sp.values)) and np.all(np.isfinite(sp.gradients))
    assert np.all(sp.normals()[0] == 0.0) and sp.status[1] == surface.CONVERGED


def _beside_the_cone(ns_, n=2048, seed=7):
    """(geometry, world points): n points within 0.05 of the inside of the cone entry's side and n within 0.05 of the
    inside of its base disc, on both sides of the surface, away from the apex and the rim."""
    make = autodiff_scenes.OP_GEOMETRIES["cone"][0]
    geo = make(ns_, *autodiff_scenes.OP_DEFAULTS)
    h, ang = autodiff_scenes._CONE
    q = np.array([h * np.tan(ang), -h])                      # the rim in the half plane (w0, w1) of prim_cone; apex (0, 0)
    normal = np.array([-q[1], q[0]]) / np.linalg.norm(q)
    rng = np.random.default_rng(seed)
    t, d = rng.uniform(0.15, 0.85, 2 * n), rng.uniform(-0.05, 0.05, 2 * n)
    phi = rng.uniform(0, 2 * np.pi, 2 * n)
    w = np.where(np.arange(2 * n) < n, t * q[:, None] + d * normal[:, None], np.stack([t * q[0], q[1] + d]))
    local = np.stack([w[0] * np.cos(phi), w[0] * np.sin(phi), w[1] + h * 0.5 ** (1.0 / 3.0)])
    return geo, autodiff_scenes.world_coordinates(geo, local).astype(np.float32)


def test_cone_normals_on_its_surface(engine):
    """A projection ends ON the surface, within 1e-7 of it after the last quadratic step. There the cone rule's residual
    to the side (and, by its rounding, to the base) is a difference of nearly equal numbers; the tangent of a free foot
    is taken from the signed form instead (csrc/sdfk_dualdev.h dual_prim_cone). Tolerance: the gradient tolerance of
    test_gpu_autodiff.py, under its kink filter. Before that change: errors of 0.5 % on the base, of order 1 on the side,
    and a zero gradient wherever f == 0."""
    geo, p = _beside_the_cone(ns)
    sp = surface.project(geo, p)
    assert np.all(sp.status == surface.CONVERGED) and sp.iterations.max() <= 2
    q = sp.points.astype(np.float64)
    D, D8 = R.gradient(geo, q), R.gradient(geo, q, R.H / 8)
    keep = np.all(np.abs(D - D8) <= 1e-7 * np.maximum(1.0, np.abs(D)), axis=0)
    err = np.abs(sp.gradients.astype(np.float64) - D).max(axis=0)
    half = p.shape[1] // 2
    print("cone: kept %.4f; max gradient error side %.3e base %.3e; |f| max %.3e"
          % (keep.mean(), err[:half][keep[:half]].max(), err[half:][keep[half:]].max(), np.abs(sp.values).max()))
    assert keep.mean() >= 0.99
    assert err[keep].max() <= 1e-4
    length = np.linalg.norm(sp.gradients.astype(np.float64), axis=0)
    assert np.abs(length - 1.0).max() <= 1e-5


# ---- 5. Lipschitz soundness -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg2", "cfg5", "cfg4"])
def test_no_point_moves_less_than_the_lipschitz_bound(engine, name):
    sp, p = _projected(name)
    lip = float(lower_geometry(_geometry(name)[0]).lipschitz)
    assert np.isfinite(lip) and lip > 0
    ok = sp.converged
    bound = (np.abs(sp.start.astype(np.float64)) - TOL) / lip - 1e-6 * np.maximum(1.0, np.abs(p).max(axis=0))
    slack = sp.distance() - bound
    print("%s: L = %g, min slack %.3e over %d converged points" % (name, lip, slack[ok].min(), ok.sum()))
    assert np.all(slack[ok] >= 0)


# ---- 6. cap on non-convergence, agreement with the float64 reference -------------------------------------------------------
@pytest.mark.parametrize("name", R.SCENES)
def test_non_convergence_is_capped_and_points_match_the_reference(engine, name):
    """Measured on an MI355X: the shares not converged equal the reference's (test_project_cpu.py) — none, 0.15 %, 0.15 %,
    0.42 % for cfg 2 / 5 / 3 / 4 —, max |q_dev - q_ref| 4.7e-5, 9.1e-6, 5.5e-6, 9.5e-7."""
    sp, p = _projected(name)
    shares = [float(np.mean(sp.status == k)) for k in range(4)]
    print("%s: converged %.4f maxiter %.4f stalled %.4f nonfinite %.4f; steps mean %.2f max %d"
          % ((name,) + tuple(shares) + (sp.iterations.mean(), sp.iterations.max())))
    ref = R.project(_geometry(name)[0], p, tol=1e-5, max_iter=32, kink_filter=True)
    both = sp.converged & (ref["status"] == R.CONVERGED) & ref["smooth"]
    err = np.abs(sp.points.astype(np.float64) - ref["points"].astype(np.float64)).max(axis=0)
    print("%s: %d points compared with the reference, max |q_dev - q_ref| %.3e" % (name, both.sum(), err[both].max()))
    assert shares[surface.NONFINITE] == 0.0
    assert 1.0 - shares[surface.CONVERGED] <= R.CAP
    assert both.sum() >= 0.5 * p.shape[1]
    assert err[both].max() <= 1e-4
    if name == "cfg4":
        assert not sp.points[2].any() and not sp.gradients[2].any()            # 2-D: z is 0 and stays 0


# ---- 7. level -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0.05, -0.05])
def test_other_levels(engine, level):
    geo, p = _geometry("cfg2")
    sp = surface.project(geo, p, level=level)
    ok = sp.converged
    print("level %g: %.4f converged" % (level, ok.mean()))
    assert ok.mean() >= 1.0 - R.CAP
    f = _create("cfg2", sp.points)
    assert np.array_equal(_bits(f), _bits(sp.values))
    assert np.all(np.abs(f[ok] - np.float32(level)) <= np.float32(TOL))
    assert np.array_equal(ok, np.abs(f - np.float32(level)) <= np.float32(TOL))


# ---- 8. sizes and the wave vote -----------------------------------------------------------------------------------------------
SENTINEL = np.float32(-12345.0)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_sizes_through_the_c_entry(engine, n):
    sp, p = _projected("cfg5")
    low, origin = autodiff._lower(_geometry("cfg5")[0], shortcuts=True)
    prog = autodiff._program(low, origin)
    L, vp = engine.lib(), engine._vp
    stride = engine.row_stride(n) + 64                     # rows wider than the points: the gaps must stay untouched
    rows = np.full((8, stride), SENTINEL, dtype=np.float32)   # q (3), gradient (3), value, start
    with engine.DeviceBuffer(3 * stride * 4) as d_co, engine.DeviceBuffer(rows.nbytes) as d_out, \
            engine.DeviceBuffer(4 * (n + 64)) as d_info:
        co = np.zeros((3, stride), dtype=np.float32)
        co[:, :n] = p[:, :n]
        d_co.upload(co)
        d_out.upload(rows)
        info = np.full(n + 64, -7, dtype=np.int32)
        d_info.upload(info)
        row = 4 * stride
        engine.check(L.sdfk_project_points_device(prog.handle, d_co.at(), n, stride, 0.0, TOL, 32, 1.0, d_out.at(), stride,
                                                  d_out.at(6 * row), d_out.at(3 * row), stride, d_out.at(7 * row),
                                                  d_info.at(), None), "sdfk_project_points_device")
        engine.check(L.sdfk_sync(None), "sdfk_sync")
        d_out.download(rows)
        d_info.download(info)
    assert np.all(rows[:, n:] == SENTINEL) and np.all(info[n:] == -7)
    got = dict(points=rows[0:3, :n], gradients=rows[3:6, :n], values=rows[6, :n], start=rows[7, :n],
               iterations=((info[:n] >> 8) & 255).astype(np.uint8), status=(info[:n] & 255).astype(np.uint8))
    _same(got, _fields(sp, slice(0, n)), "n = %d" % n)
    assert np.all(info[:n] >> 16 == 0)


def test_a_slow_lane_does_not_disturb_its_wave(engine):
    sp, p = _projected("cfg5")
    slow = np.flatnonzero(sp.iterations > 4)
    fast = np.flatnonzero((sp.iterations == 1) & sp.converged)
    assert slow.size >= 1 and fast.size >= 63
    pick = np.concatenate([fast[:20], slow[:1], fast[20:63]])
    geo = _geometry("cfg5")[0]
    wave = surface.project(geo, p[:, pick])
    assert np.count_nonzero(wave.iterations > 4) == 1 and np.count_nonzero(wave.iterations == 1) == 63
    _same(_fields(wave), _fields(sp, pick), "the wave against the 4096-point run")
    for k, i in enumerate(pick):
        alone = surface.project(geo, p[:, i:i + 1])
        _same(_fields(alone), _fields(wave, slice(k, k + 1)), "point %d alone" % i)


@pytest.mark.parametrize("name", ["cfg5", "cfg3"])
def test_a_permutation_permutes_the_result(engine, name):
    sp, p = _projected(name)
    perm = np.random.default_rng(11).permutation(p.shape[1])
    got = surface.project(_geometry(name)[0], np.ascontiguousarray(p[:, perm]))
    _same(_fields(got), _fields(sp, perm), name)


# ---- 9. resident --------------------------------------------------------------------------------------------------------------
class CountingLib:
    """The library, with the live device allocations of the Python layer counted (as the stand-in device of
    test_device_buffers_cpu.py counts them)."""

    def __init__(self, real):
        self.real, self.live, self.bad_frees, self.mallocs = real, set(), [], 0

    def sdfk_malloc(self, nbytes):
        p = self.real.sdfk_malloc(nbytes)
        if p:
            self.mallocs += 1
            self.live.add(p)
        return p

    def sdfk_free(self, p):
        a = (p.value if isinstance(p, ctypes.c_void_p) else p) or 0
        if a in self.live:
            self.live.remove(a)
        else:
            self.bad_frees.append(a)
        return self.real.sdfk_free(p)

    def __getattr__(self, name):
        return getattr(self.real, name)


def test_resident_rows_equal_the_host_path_and_are_released(engine):
    sp, p = _projected("cfg5")
    geo = _geometry("cfg5")[0]
    gc.collect()
    real = engine.lib()
    counting = CountingLib(real)
    engine._lib = counting
    try:
        d_p = engine.DeviceVectorField.from_host(p)
        res = surface.project(geo, d_p, resident=True)
        assert isinstance(res.points, engine.DeviceVectorField) and isinstance(res.gradients, engine.DeviceVectorField)
        assert isinstance(res.values, engine.DeviceField) and isinstance(res.start, engine.DeviceField)
        assert res.origin is None and len(counting.live) == 5
        got = dict(points=res.points.numpy(), values=res.values.numpy(), gradients=res.gradients.numpy(),
                   start=res.start.numpy(), iterations=res.iterations, status=res.status)
        _same(got, _fields(sp), "resident in and out")
        assert np.array_equal(res.normals(), sp.normals()) and np.array_equal(res.distance(d_p), sp.distance())
        again = surface.project(geo, res.points, max_iter=0)              # a resident result is an input
        assert np.array_equal(_bits(again.points), _bits(sp.points)) and np.array_equal(_bits(again.values), _bits(sp.values))
        assert len(counting.live) == 5
        host_in = surface.project(geo, p, resident=True)
        assert np.array_equal(_bits(host_in.points.numpy()), _bits(sp.points)) and len(counting.live) == 9
        host_in.free()
        res.free()
        d_p.free()
        gc.collect()
        assert not counting.live and not counting.bad_frees and counting.mallocs > 9
    finally:
        engine._lib = real


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------------
def test_trees_without_a_dual_rule_are_refused(engine):
    p = R.scene_points((2.0, 2.0, 2.0), n=64)
    with pytest.raises(autodiff.UnsupportedOpError, match="P_BRAID"):
        surface.project(ns.Braid(1.0, 0.3, 0.1, 1.0), p)
    signed = ns.Circle(0.5)
    signed.signed((32, 32, 1))
    with pytest.raises(autodiff.UnsupportedOpError, match="staged"):
        surface.project(signed, p)


# ---- 11. consumers --------------------------------------------------------------------------------------------------------------
def _vertex_field(geometry, vertices):
    co = np.zeros((3, len(vertices)), dtype=np.float32)
    co[:vertices.shape[1]] = vertices.T
    return _create(geometry, co)


def test_mesh_project_polishes_a_coarse_sphere(engine):
    m = mesh.from_geometry(ns.Sphere(0.5), (2, 2, 2), (33, 33, 33))
    faces, before = m.faces.copy(), m.vertices.copy()
    off = np.abs(_vertex_field(ns.Sphere(0.5), before)).max()
    assert off > 1e-4
    sp = m.project(ns.Sphere(0.5))
    assert isinstance(sp, surface.SurfacePoints) and np.all(sp.status == surface.CONVERGED)
    after = np.abs(_vertex_field(ns.Sphere(0.5), m.vertices)).max()
    print("sphere mesh, %d vertices: max |f| %.3e before, %.3e after" % (len(before), off, after))
    assert after <= TOL
    assert np.array_equal(m.faces, faces) and m.vertices.shape == before.shape and m.vertices.dtype == np.float32
    assert np.array_equal(_bits(m.vertices), _bits(np.ascontiguousarray(sp.points.T)))
    g = sp.gradients.astype(np.float64).T
    assert np.array_equal(m.normals, (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32))
    assert np.array_equal(m.normals, sp.normals())


def test_mesh_project_leaves_unconverged_vertices_of_cfg2(engine):
    geo = _geometry("cfg2")[0]
    m = mesh.from_geometry(geo, (2, 2, 2), (65, 65, 65))
    faces, before = m.faces.copy(), m.vertices.copy()
    sp = m.project(_geometry("cfg2")[0])
    ok = sp.converged
    print("cfg2 mesh, %d vertices: %.4f converged" % (len(before), ok.mean()))
    assert ok.mean() >= 0.99
    assert np.array_equal(_bits(m.vertices[~ok]), _bits(before[~ok]))
    assert np.array_equal(_bits(m.vertices[ok]), _bits(np.ascontiguousarray(sp.points.T[ok])))
    assert np.abs(_vertex_field("cfg2", m.vertices)[ok]).max() <= TOL
    assert np.array_equal(m.faces, faces) and np.array_equal(m.normals, sp.normals())


def test_contour_project_stays_in_the_plane(engine):
    c = mesh.from_geometry(ns.Circle(0.4), (2, 2), (65, 65))
    segments, before = c.segments.copy(), c.vertices.copy()
    assert before.shape[1] == 2 and np.abs(_vertex_field(ns.Circle(0.4), before)).max() > 1e-5
    sp = c.project(ns.Circle(0.4))
    assert not sp.origin[2].any() and not sp.points[2].any() and not sp.gradients[2].any()
    assert np.all(sp.status == surface.CONVERGED) and c.vertices.shape == before.shape
    assert np.abs(_vertex_field(ns.Circle(0.4), c.vertices)).max() <= TOL
    assert np.abs(np.hypot(c.vertices[:, 0].astype(np.float64), c.vertices[:, 1].astype(np.float64)) - 0.4).max() <= 2 * TOL
    assert np.array_equal(c.segments, segments) and np.array_equal(c.normals, sp.normals()) and not c.normals[:, 2].any()
