"""GPU: forward-mode derivatives (aegolius_amd.autodiff) against float64 central differences of the CPU oracle, the value
channel against create(), channel grouping, the spatial gradient, the post-processing chain rule and an end-to-end
gradient descent (the reference's position_optimization example)."""
import numpy as np
import pytest

import aegolius_amd.cores as ns
import autodiff_scenes
from aegolius_amd import _engine, autodiff as ad
from aegolius_amd._lower import lower_geometry
from oracle import sdf_oracle

pytestmark = pytest.mark.gpu


def _points(seed=5, n=4096, extent=1.6, dim=3):
    rng = np.random.default_rng(seed)
    co = rng.uniform(-extent, extent, (3, n))
    if dim == 2:
        co[2] = 0.0
    return co.astype(np.float32).astype(np.float64)


def _is_2d(name):
    return name in autodiff_scenes.AUTODIFF_SCRIPTS and name != "gradient_map_3D" or name in (
        "fam_2d_prims", "fam_2d_arc_segment", "fam_triangle_smax_parameters")


def _reference(builder, primals, a, i, co):
    """float64 central difference of the oracle at p +- h (h = 1e-6 max(1, |p|)), and the mask of points where the
    differences at h and h/8 agree (kink filter)."""
    p = float(np.asarray(primals[a], dtype=np.float64).ravel()[0 if i is None else i])

    def diff(h):
        f = [sdf_oracle.evaluate(builder(*ad._moved(primals, a, i, s * h)), co) for s in (1.0, -1.0)]
        return (f[0] - f[1]) / (2 * h)
    h = 1e-6 * max(1.0, abs(p))
    D, D8 = diff(h), diff(h / 8)
    keep = np.abs(D - D8) <= 1e-7 * np.maximum(1.0, np.abs(D))
    return D, keep


def _spatial_reference(geo, co, ax):
    """float64 central difference of the oracle along axis `ax` at h = 1e-6, and the kink filter: the points where it
    agrees with the difference at h / 8."""
    def moved(d):
        c = co.copy()
        c[ax] += d
        return sdf_oracle.evaluate(geo, c)
    h = 1e-6
    D = (moved(h) - moved(-h)) / (2 * h)
    D8 = (moved(h / 8) - moved(-h / 8)) / (h / 4)
    keep = np.abs(D - D8) <= 1e-7 * np.maximum(1.0, np.abs(D))
    return D, keep


def _check(t, D, keep, what):
    assert keep.mean() >= 0.90, "%s: only %.1f %% of the points kept" % (what, 100 * keep.mean())
    err = np.abs(t.astype(np.float64) - D)[keep] / np.maximum(1.0, np.abs(D[keep]))
    assert np.all(np.isfinite(t)), what
    assert err.max() <= 1e-4, "%s: max rel err %.3e" % (what, err.max())
    assert np.percentile(err, 99) <= 1e-5, "%s: p99 rel err %.3e" % (what, np.percentile(err, 99))


@pytest.mark.parametrize("name", sorted(autodiff_scenes.SCENES))
def test_jacobian_matches_oracle_differences(name, engine):
    fn, primals, argnums = autodiff_scenes.SCENES[name]
    builder = fn(ns)
    ref_builder = fn(ns)
    co = _points(dim=2 if _is_2d(name) else 3, n=2048 if name == "cfg2_width" else 4096)
    value, jac = ad.value_and_jacfwd(builder, co, primals, argnums)
    jacs = (jac,) if isinstance(argnums, int) else jac
    nums = (argnums,) if isinstance(argnums, int) else argnums
    for a, J in zip(nums, jacs):
        arr = np.asarray(primals[a], dtype=np.float64)
        rows = [J] if arr.ndim == 0 else list(J)
        for i, t in enumerate(rows):
            D, keep = _reference(ref_builder, primals, a, None if arr.ndim == 0 else i, co)
            _check(t, D, keep, "%s argnum %d[%d]" % (name, a, i))


def test_circle_radius_derivative_is_exactly_minus_one(engine):
    """gradient_map_parameters: d circle / d r = -1 at every point of the 401 x 401 grid."""
    co, _res = ns.generate_grid((4, 4), (400, 400))
    value, jac = ad.value_and_jacfwd(lambda r: ns.Circle(r), co, (1.0,), 0)
    assert jac.shape == (160801,)
    assert np.all(jac == np.float32(-1.0))
    np.testing.assert_array_equal(value, ns.Circle(1.0).create(co))


def test_value_channel_equals_create_bit_for_bit(engine):
    """The value channel is the field the evaluation kernels give for the same (shortcut-free) program, bit for bit, on
    every scene. create() itself lowers with the shortcuts (identity transforms aliased ...), so its program is a different
    one on these scenes; where the two programs are the same — a geometry whose every node carries a transform that no
    shortcut removes — the value channel is create()'s field."""
    for name in sorted(autodiff_scenes.SCENES):
        fn, primals, argnums = autodiff_scenes.SCENES[name]
        builder = fn(ns)
        co = _points(seed=9, dim=2 if _is_2d(name) else 3, n=1000)
        value, _ = ad.value_and_jacfwd(builder, co, primals, argnums)
        low_free = lower_geometry(builder(*primals), shortcuts=False)
        same_prog = _engine.Program(low_free.code, low_free.params, low_free.tables, low_free.result_reg)
        np.testing.assert_array_equal(value, same_prog.eval_host(co), err_msg=name)

    def placed(r):
        s = ns.Sphere(r)
        s.rotate(0.3, (1, 2, 3))
        s.set_scale(1.5)
        return s
    low, low_free = lower_geometry(placed(0.5)), lower_geometry(placed(0.5), shortcuts=False)
    assert np.array_equal(low.code, low_free.code) and np.array_equal(low.params, low_free.params)
    co = _points(seed=3)
    value, _ = ad.value_and_jacfwd(placed, co, (0.5,), 0)
    np.testing.assert_array_equal(value, placed(0.5).create(co))


def test_grouped_channels_equal_single_channels(engine):
    fn, primals, argnums = autodiff_scenes.SCENES["gradient_map_combine"]
    builder = fn(ns)
    co = _points(seed=11, dim=2)
    _v, jac4 = ad.value_and_jacfwd(builder, co, primals, (0, 1, 2, 3))
    for k in range(4):
        _v1, one = ad.value_and_jacfwd(builder, co, primals, k)
        np.testing.assert_array_equal(jac4[k], one)
    fn, primals, argnums = autodiff_scenes.SCENES["multi_position_optimization"]
    builder = fn(ns)
    _v, (jx, jy) = ad.value_and_jacfwd(builder, co, primals, (0, 1))      # 6 channels: two launches
    _v, jx1 = ad.value_and_jacfwd(builder, co, primals, 0)
    _v, jy1 = ad.value_and_jacfwd(builder, co, primals, 1)
    np.testing.assert_array_equal(jx, jx1)
    np.testing.assert_array_equal(jy, jy1)


def test_jvp_is_the_contraction_of_the_jacobian(engine):
    fn, primals, argnums = autodiff_scenes.SCENES["gradient_map_combine"]
    builder = fn(ns)
    co = _points(seed=12, dim=2)
    _v, jac = ad.value_and_jacfwd(builder, co, primals, argnums)
    direction = (0.5, -1.0, 0.0, 2.0)
    _v, t = ad.jvp(builder, co, primals, direction)
    want = sum(w * j.astype(np.float64) for w, j in zip(direction, jac))
    np.testing.assert_allclose(t, want, rtol=1e-5, atol=1e-5)


def test_spatial_gradient(engine):
    geo = autodiff_scenes.SCENES["fam_torus_chainlink_cone"][0](ns)(0.3, 0.1, 0.6)
    co = _points(seed=13)
    value, g = ad.value_and_grad_points(geo, co)
    np.testing.assert_array_equal(value, geo.create(co))
    for ax in range(3):
        def moved(d, ax=ax):
            c = co.copy()
            c[ax] += d
            return sdf_oracle.evaluate(geo, c)
        h = 1e-6
        D = (moved(h) - moved(-h)) / (2 * h)
        D8 = (moved(h / 8) - moved(-h / 8)) / (h / 4)
        keep = np.abs(D - D8) <= 1e-7 * np.maximum(1.0, np.abs(D))
        _check(g[ax], D, keep, "axis %d" % ax)
    s = ns.Sphere(0.7)
    s.move((0.1, -0.2, 0.3))
    pts = _points(seed=14)
    pts = pts[:, np.linalg.norm(pts - np.array([[0.1], [-0.2], [0.3]]), axis=0) > 0.05]
    _v, g = ad.value_and_grad_points(s, pts)
    np.testing.assert_allclose(np.linalg.norm(g.astype(np.float64), axis=0), 1.0, atol=1e-6)


@pytest.mark.parametrize("name", sorted(autodiff_scenes.POINT_SCENES))
def test_spatial_gradient_of_default_programs(name, engine):
    """Point mode on the default lowering, including the ops only it emits (MOVC, VEXPFLAG)."""
    geo = autodiff_scenes.POINT_SCENES[name](ns)
    co = _points(seed=15)
    value, g = ad.value_and_grad_points(geo, co)
    np.testing.assert_array_equal(value, geo.create(co))
    for ax in range(3):
        def moved(d, ax=ax):
            c = co.copy()
            c[ax] += d
            return sdf_oracle.evaluate(geo, c)
        h = 1e-6
        D = (moved(h) - moved(-h)) / (2 * h)
        D8 = (moved(h / 8) - moved(-h / 8)) / (h / 4)
        keep = np.abs(D - D8) <= 1e-7 * np.maximum(1.0, np.abs(D))
        _check(g[ax], D, keep, "%s axis %d" % (name, ax))


def _op_builder(name):
    make = autodiff_scenes.OP_GEOMETRIES[name][0]
    return lambda tx, ty, ang, s: make(ns, tx, ty, ang, s)


@pytest.mark.parametrize("name", sorted(autodiff_scenes.OP_GEOMETRIES))
def test_spatial_gradient_of_every_op(name, engine):
    """∇_x of one geometry per dual rule behind a skew placement (every input-tangent term with all components live),
    on the default lowering, against central differences of the oracle; the value is create()'s bit for bit."""
    _make, dim, _targets, _regions = autodiff_scenes.OP_GEOMETRIES[name]
    geo = _op_builder(name)(*autodiff_scenes.OP_DEFAULTS)
    co = _points(seed=15, dim=dim)
    value, g = ad.value_and_grad_points(geo, co)
    np.testing.assert_array_equal(value, geo.create(co))
    for ax in range(3):
        D, keep = _spatial_reference(geo, co, ax)
        if dim == 2 and ax == 2:
            assert np.all(g[ax][D == 0.0] == 0.0), "%s: the z row of a 2-D geometry" % name
        if name in autodiff_scenes.ZERO_TANGENT_ENTRIES:
            assert np.all(g[ax][D == 0.0] == 0.0), "%s axis %d: the tangent of a piecewise-constant map" % (name, ax)
        _check(g[ax], D, keep, "%s axis %d" % (name, ax))


@pytest.mark.parametrize("name", sorted(autodiff_scenes.NORMAL_POINTS))
def test_spatial_gradient_beside_the_normals_at_corners(name, engine):
    """Points at 1e-4 to 3e-3 rad from the normal erected where two pieces of the boundary meet (every vertex of the
    triangle, the rim of the cone), 0.005 to 0.5 piece lengths away, on the side of the piece with the free foot. There
    the two pieces' squared distances tie in fp32 and their gradients differ by the angle, 30 times the bound at the most:
    a rule that picks by the squared distance alone fails (the triangle's did, by up to 3e-3)."""
    geo = _op_builder(name)(*autodiff_scenes.OP_DEFAULTS)
    co = autodiff_scenes.world_coordinates(geo, autodiff_scenes.NORMAL_POINTS[name]())
    co = co.astype(np.float32).astype(np.float64)
    value, g = ad.value_and_grad_points(geo, co)
    np.testing.assert_array_equal(value, geo.create(co))
    for ax in range(3):
        D, keep = _spatial_reference(geo, co, ax)
        _check(g[ax], D, keep, "%s axis %d" % (name, ax))


@pytest.mark.parametrize("name", sorted(autodiff_scenes.OP_GEOMETRIES))
def test_placement_jacobian_of_every_op(name, engine):
    """d/d(tx, ty, ang, s) of the same geometries: the input-tangent terms again, through the K = 4 parameter-mode
    instantiation, fed by XFORM's parameter tangents (one launch)."""
    dim = autodiff_scenes.OP_GEOMETRIES[name][1]
    builder, primals = _op_builder(name), autodiff_scenes.OP_DEFAULTS
    co = _points(seed=15, dim=dim)
    value, jac = ad.value_and_jacfwd(builder, co, primals, (0, 1, 2, 3))
    assert np.all(np.isfinite(value))
    for a, t in enumerate(jac):
        D, keep = _reference(_op_builder(name), primals, a, None, co)
        if name in autodiff_scenes.ZERO_TANGENT_ENTRIES:
            assert np.all(t[D == 0.0] == 0.0), "%s argnum %d: the tangent of a piecewise-constant map" % (name, a)
        _check(t, D, keep, "%s argnum %d" % (name, a))


@pytest.mark.parametrize("name", sorted(autodiff_scenes.OP_GEOMETRIES))
def test_derivatives_are_finite_on_a_grid_through_the_origin(name, engine):
    """Identity placement and a grid with nodes exactly on the rules' ties (x == 0, |x| == |y|, the ends of the repeated
    spans, sector boundaries): the value, ∇_x, the four-channel Jacobian and the vjp are finite for every rule. The
    placement keeps its constant z offset, so a 3-D entry runs a second time on the grid moved by that offset, whose
    nodes then sit on the ties in z as well (z == 0, the caps, the ends of a span along z)."""
    dim = autodiff_scenes.OP_GEOMETRIES[name][1]
    co, _res = ns.generate_grid((2, 2, 2), (20, 20, 20)) if dim == 3 else ns.generate_grid((2, 2), (20, 20))
    builder, primals = _op_builder(name), autodiff_scenes.OP_IDENTITY
    grids = [co]
    if dim == 3:
        moved = np.array(co, dtype=np.float64)
        moved[2] += autodiff_scenes.PLACE_Z
        grids.append(moved)
    for co in grids:
        value, g = ad.value_and_grad_points(builder(*primals), co)
        assert np.all(np.isfinite(value)) and np.all(np.isfinite(g))
        value, jac = ad.value_and_jacfwd(builder, co, primals, (0, 1, 2, 3))
        assert np.all(np.isfinite(value)) and np.all(np.isfinite(np.stack(jac)))
        c = np.random.default_rng(17).normal(size=value.size).astype(np.float32)
        v, grads = ad.vjp(builder, co, primals, c, (0, 1, 2, 3))
        assert np.all(np.isfinite(v)) and np.all(np.isfinite(np.array(grads, dtype=np.float64)))


def test_no_nan_at_centres_and_axes(engine):
    co, _res = ns.generate_grid((2, 2, 2), (20, 20, 20))        # passes through 0 on every axis
    for geo_fn, primals in ((lambda r: ns.Circle(r), (0.5,)), (lambda r: ns.Sphere(r), (0.5,)),
                            (lambda r: ns.Torus(r, 0.1), (0.5,)), (lambda r: ns.Cylinder(r, 0.6), (0.3,))):
        value, jac = ad.value_and_jacfwd(geo_fn, co, primals, 0)
        assert np.all(np.isfinite(jac)) and np.all(np.isfinite(value))
        _v, g = ad.value_and_grad_points(geo_fn(*primals), co)
        assert np.all(np.isfinite(g))


def _post_ref(name, v, params):
    """float64 analytic derivative of the map in its first argument."""
    v = v.astype(np.float64)
    if name == "sigmoid_falloff":
        A, w = params
        e = np.exp(4 * v / w)
        return -A * (4 / w) * e / (1 + e) ** 2
    if name == "positive_sigmoid_falloff":
        A, w = params
        e = np.exp(4 * (v - w) / w)
        return -A * (4 / w) * e / (1 + e) ** 2
    if name == "capped_exponential":
        A, w = params
        e = np.exp(-4 * v / w)
        return np.where(e < 1, -A * 4 / w * e, 0.0)
    if name == "hard_binarization":
        return np.zeros_like(v)
    if name == "linear_falloff":
        A, w = params
        t = 1 - v / w
        return np.where((t > 0) & (t < 1), -A / w, 0.0)
    if name == "relu":
        w, = params
        return np.where(v > 0, 1 / w, 0.0)
    if name == "smooth_relu":
        sw, w, thr = params
        b = (sw + thr) * 4 * thr
        u = v / w
        return 0.5 * (1 + u / np.sqrt(u * u + b)) / w
    if name == "slowstart":
        sw, w, thr, ground = params
        b = (2 * sw + thr) * thr / w
        u = np.maximum(v / w, 0)
        return np.where(v > 0, u / np.sqrt(u * u + b) / w, 0.0)
    A, w = params
    u = np.maximum(v, 0) if name == "gaussian_falloff" else v
    d = A * np.exp(-4 * (u / w) ** 2) * (-8 * u / w ** 2)
    return np.where(v > 0, d, 0.0) if name == "gaussian_falloff" else d


POST = {"sigmoid_falloff": (1.0, 0.5), "positive_sigmoid_falloff": (1.0, 0.5), "capped_exponential": (1.0, 0.5),
        "hard_binarization": (0.0,), "linear_falloff": (1.0, 0.5), "relu": (0.7,), "smooth_relu": (0.2, 0.8, 0.01),
        "slowstart": (0.2, 0.8, 0.01, True), "gaussian_boundary": (1.0, 0.5), "gaussian_falloff": (1.0, 0.5)}


@pytest.mark.parametrize("name", sorted(POST))
def test_post_jvp(name, engine):
    from aegolius_amd.cores import post_processing
    rng = np.random.default_rng(21)
    v = rng.uniform(-1.5, 1.5, 5000).astype(np.float32)
    v = v[np.abs(v) > 1e-3]
    t = rng.uniform(-2, 2, v.size).astype(np.float32)
    params = POST[name]
    out, out_t = ad.post_jvp(name, v, t, *params)
    np.testing.assert_array_equal(out, getattr(post_processing, name)(v, *params))
    want = _post_ref(name, v, params) * t.astype(np.float64)
    err = np.abs(out_t - want) / np.maximum(1.0, np.abs(want))
    assert err.max() <= 1e-5, err.max()
    dv, dt = _engine.DeviceField.from_host(v), _engine.DeviceField.from_host(t)
    rv, rt = ad.post_jvp(name, dv, dt, *params)
    np.testing.assert_array_equal(rv.numpy(), out)
    np.testing.assert_array_equal(rt.numpy(), out_t)


def test_resident_equals_host(engine):
    fn, primals, argnums = autodiff_scenes.SCENES["gradient_map_transformations"]
    builder = fn(ns)
    co, _res = ns.generate_grid((4, 4), (64, 64))
    value, (jx, jy, jr) = ad.value_and_jacfwd(builder, co, primals, argnums)
    dco = _engine.DeviceVectorField.from_host(np.asarray(co))
    rv, (rx, ry, rr) = ad.value_and_jacfwd(builder, dco, primals, argnums, resident=True)
    assert isinstance(rv, _engine.DeviceField)
    np.testing.assert_array_equal(rv.numpy(), value)
    for a, b in ((rx, jx), (ry, jy), (rr, jr)):
        np.testing.assert_array_equal(a.numpy(), b)
    assert rv.select(0.0).size == np.count_nonzero(value <= 0)


def test_position_optimization_converges(engine):
    """examples/autodiff/position_optimization.py: gradient descent on the circle centre against a target field of
    gaussian-falloff circles, gradient of the sum of squared differences through value_and_jacfwd."""
    co, _res = ns.generate_grid((8, 8), (100, 100))
    build = autodiff_scenes.SCENES["position_optimization"][0](ns)
    target = build(2.5, -1.0).create(co).astype(np.float64)
    x = np.array([1.8, -0.4])
    lr = None
    for _ in range(400):
        f, (jx, jy) = ad.value_and_jacfwd(build, co, (x[0], x[1]), (0, 1))
        r = f.astype(np.float64) - target
        J = np.stack([jx, jy]).astype(np.float64)
        g = 2 * J.dot(r)
        if lr is None:                                   # one fixed step: 1 / the largest curvature at the start
            lr = 1.0 / np.linalg.eigvalsh(2 * J.dot(J.T)).max()
        x = x - lr * g
        if np.linalg.norm(x - [2.5, -1.0]) < 1e-4:
            break
    assert np.linalg.norm(x - [2.5, -1.0]) < 1e-3, x
