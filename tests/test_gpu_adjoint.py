"""GPU: reverse-mode derivatives (aegolius_amd.autodiff.vjp / value_and_grad_sse) against the float64 contraction of the
forward-mode Jacobian, on the default and the generic-rule paths, against central differences of the oracle's loss, the
value and loss outputs, determinism, edge sizes, resident I/O, the largest accepted program, and two replays of the
reference's optimisation examples."""
import numpy as np
import pytest

import aegolius_amd.cores as ns
import autodiff_scenes
from aegolius_amd import _engine, autodiff as ad
from oracle import sdf_oracle
from test_adjoint_cpu import _circles, largest_program

pytestmark = pytest.mark.gpu


def _points(seed=5, n=4096, extent=1.6, dim=3):
    rng = np.random.default_rng(seed)
    co = rng.uniform(-extent, extent, (3, n))
    if dim == 2:
        co[2] = 0.0
    return co.astype(np.float32).astype(np.float64)


def _is_2d(name):
    return name in autodiff_scenes.AUTODIFF_SCRIPTS and name != "gradient_map_3D" or name in ("fam_2d_prims", "fam_2d_arc_segment")


def _flat(grads):
    parts = grads if isinstance(grads, tuple) else (grads,)
    return np.concatenate([np.atleast_1d(np.asarray(g, dtype=np.float64)) for g in parts])


def _jac_rows(jac, primals, argnums):
    jacs = jac if isinstance(argnums, tuple) else (jac,)
    nums = argnums if isinstance(argnums, tuple) else (argnums,)
    rows = []
    for a, J in zip(nums, jacs):
        rows.extend([J] if np.ndim(primals[a]) == 0 else list(J))
    return np.array(rows, dtype=np.float64).reshape(len(rows), -1)


def _contraction(builder, co, primals, argnums, c):
    """(Σ_i c_i J_ki, Σ_i |c_i J_ki|, value) from value_and_jacfwd, in float64."""
    value, jac = ad.value_and_jacfwd(builder, co, primals, argnums)
    J = _jac_rows(jac, primals, argnums)
    c = np.asarray(c, dtype=np.float64)
    return J.dot(c), np.abs(J).dot(np.abs(c)), value


def _parameter_scale(builder, co, primals, argnums, c):
    """Σ_j |P̄_j dP_j/dθ_k|: the size of the terms the host chain rule adds. Where they cancel to a derivative that is
    zero in exact arithmetic (a sphere turned about its centre), both modes return rounding noise of this size."""
    low, origin, rows, _chans, _layout = ad.parameter_tangents(builder, primals, argnums)
    v, pbar, _loss = ad._reverse(ad._adjoint_program(low, origin), co, c, 0, True, low.params.size)
    v.free()
    return np.abs(rows).dot(np.abs(pbar))


def _close(got, want, scale, what):
    bound = 1e-5 * scale + 1e-7
    err = np.abs(got - want)
    assert np.all(err <= bound), "%s: err %s > bound %s" % (what, err, bound)


@pytest.mark.parametrize("name", sorted(autodiff_scenes.SCENES))
def test_vjp_matches_the_forward_contraction(name, engine):
    fn, primals, argnums = autodiff_scenes.SCENES[name]
    builder = fn(ns)
    co = _points(dim=2 if _is_2d(name) else 3)
    c = np.random.default_rng(17).normal(size=co.shape[1]).astype(np.float32)
    want, scale, value = _contraction(builder, co, primals, argnums, c)
    scale = np.maximum(scale, 1e-2 * _parameter_scale(builder, co, primals, argnums, c))
    v, g = ad.vjp(builder, co, primals, c, argnums)
    vg, gg = ad.vjp(builder, co, primals, c, argnums, generic_rules=True)
    np.testing.assert_array_equal(v, value)
    np.testing.assert_array_equal(vg, value)
    _close(_flat(g), want, scale, name + " default rules")
    _close(_flat(gg), want, scale, name + " generic rules")
    _close(_flat(g), _flat(gg), scale, name + " default against generic")


def _param_contraction(prog, co, c, n_params):
    """Σ_i c_i ∂f_i/∂P_j for every parameter j, from forward mode seeded with unit rows."""
    rows = np.eye(n_params, dtype=np.float32)
    _v, tans = ad._evaluate_channels(prog, co, rows, False)
    T = np.array(tans, dtype=np.float64)
    c = c.astype(np.float64)
    return T.dot(c), np.abs(T).dot(np.abs(c))


@pytest.mark.parametrize("name", sorted(autodiff_scenes.POINT_SCENES))
def test_parameter_adjoints_of_default_programs(name, engine):
    """P̄ itself on the default lowering (the ops only it emits: MOVC, VEXPFLAG), both paths, against forward mode."""
    geo = autodiff_scenes.POINT_SCENES[name](ns)
    low, origin = ad._lower(geo, shortcuts=True)
    prog = ad._adjoint_program(low, origin)
    co = _points(seed=15, n=2048)
    c = np.random.default_rng(4).normal(size=co.shape[1]).astype(np.float32)
    want, scale = _param_contraction(prog, co, c, low.params.size)
    for generic in (False, True):
        v, pbar, _loss = ad._reverse(prog, co, c, 0, generic, low.params.size)
        v.free()
        _close(pbar, want, scale, "%s generic=%s" % (name, generic))


@pytest.mark.parametrize("name", sorted(autodiff_scenes.OP_GEOMETRIES))
def test_vjp_of_every_op_placement(name, engine):
    """Reverse mode over the placement (tx, ty, ang, s) of one geometry per rule: the adjoint's input-coordinate products
    of every rule are consumed by XFORM's parameters, and agree with forward mode (which test_gpu_autodiff anchors to the
    oracle) on both paths."""
    make, dim, _targets, _regions = autodiff_scenes.OP_GEOMETRIES[name]

    def builder(tx, ty, ang, s):
        return make(ns, tx, ty, ang, s)
    primals, argnums = autodiff_scenes.OP_DEFAULTS, (0, 1, 2, 3)
    co = _points(seed=15, dim=dim)
    c = np.random.default_rng(17).normal(size=co.shape[1]).astype(np.float32)
    want, scale, value = _contraction(builder, co, primals, argnums, c)
    scale = np.maximum(scale, 1e-2 * _parameter_scale(builder, co, primals, argnums, c))
    v, g = ad.vjp(builder, co, primals, c, argnums)
    vg, gg = ad.vjp(builder, co, primals, c, argnums, generic_rules=True)
    np.testing.assert_array_equal(v, value)
    np.testing.assert_array_equal(vg, value)
    _close(_flat(g), want, scale, name + " default rules")
    _close(_flat(gg), want, scale, name + " generic rules")
    _close(_flat(g), _flat(gg), scale, name + " default against generic")


@pytest.mark.parametrize("name", sorted(autodiff_scenes.OP_GEOMETRIES))
def test_parameter_adjoints_of_every_op(name, engine):
    """P̄ of every parameter of the default lowering of one geometry per rule, both paths, against forward mode."""
    make, dim, _targets, _regions = autodiff_scenes.OP_GEOMETRIES[name]
    geo = make(ns, *autodiff_scenes.OP_DEFAULTS)
    low, origin = ad._lower(geo, shortcuts=True)
    prog = ad._adjoint_program(low, origin)
    co = _points(seed=15, n=2048, dim=dim)
    c = np.random.default_rng(4).normal(size=co.shape[1]).astype(np.float32)
    want, scale = _param_contraction(prog, co, c, low.params.size)
    for generic in (False, True):
        v, pbar, _loss = ad._reverse(prog, co, c, 0, generic, low.params.size)
        v.free()
        _close(pbar, want, scale, "%s generic=%s" % (name, generic))


def _oracle_loss(builder, primals, co, target):
    f = sdf_oracle.evaluate(builder(*primals), co)
    return float(np.sum((f - target) ** 2))


@pytest.mark.parametrize("name", ["multi_position_optimization", "gradient_map_combine", "fam_sphere_box_cyl"])
def test_sse_gradient_matches_oracle_loss_differences(name, engine):
    fn, primals, argnums = autodiff_scenes.SCENES[name]
    builder, ref = fn(ns), fn(ns)
    co = _points(seed=6, dim=2 if _is_2d(name) else 3)
    moved = tuple(np.asarray(p, dtype=np.float64) + 0.05 for p in primals)
    target = builder(*moved).create(co).astype(np.float64)
    loss, g = ad.value_and_grad_sse(builder, co, primals, target, argnums)
    got = _flat(g)
    chans, _layout = ad.channel_layout(primals, argnums)
    D = []
    for a, i in chans:
        p = float(np.asarray(primals[a], dtype=np.float64).ravel()[0 if i is None else i])
        h = 1e-6 * max(1.0, abs(p))
        lp = _oracle_loss(ref, ad._moved(primals, a, i, h), co, target.astype(np.float32))
        lm = _oracle_loss(ref, ad._moved(primals, a, i, -h), co, target.astype(np.float32))
        D.append((lp - lm) / (2 * h))
    D = np.array(D)
    err = np.abs(got - D)
    assert np.all(err <= 1e-4 * np.maximum(np.abs(D), np.abs(D).max())), (name, got, D)


def test_value_and_loss_outputs(engine):
    fn, primals, argnums = autodiff_scenes.SCENES["gradient_map_3D"]
    builder = fn(ns)
    co = _points(seed=7)
    value, _jac = ad.value_and_jacfwd(builder, co, primals, argnums)
    target = np.random.default_rng(8).normal(size=co.shape[1]).astype(np.float32)
    v, _g = ad.vjp(builder, co, primals, target, argnums)
    np.testing.assert_array_equal(v, value)
    loss, _g = ad.value_and_grad_sse(builder, co, primals, target, argnums)
    want = np.sum((value.astype(np.float64) - target.astype(np.float64)) ** 2)
    assert abs(loss - want) <= 1e-6 * want


def test_two_calls_give_identical_bits(engine):
    fn, primals, argnums = autodiff_scenes.SCENES["fam_value_maps"]
    builder = fn(ns)
    co, _res = ns.generate_grid((3, 3, 3), (90, 90, 90))        # 91^3: many workgroups per grid slot
    target = np.random.default_rng(9).normal(size=91 ** 3).astype(np.float32)
    l1, g1 = ad.value_and_grad_sse(builder, co, primals, target, argnums)
    l2, g2 = ad.value_and_grad_sse(builder, co, primals, target, argnums)
    assert np.float64(l1).tobytes() == np.float64(l2).tobytes()
    assert _flat(g1).tobytes() == _flat(g2).tobytes()
    _v, g3 = ad.vjp(builder, co, primals, target, argnums)
    _v, g4 = ad.vjp(builder, co, primals, target, argnums)
    assert _flat(g3).tobytes() == _flat(g4).tobytes()


@pytest.mark.parametrize("n", [0, 1, 1000, 2048 * 256 + 777])
def test_edge_sizes(n, engine):
    """N = 0, N = 1, a partial workgroup, and more points than the persistent grid covers in one stride."""
    fn, primals, argnums = autodiff_scenes.SCENES["gradient_map_combine"]
    builder = fn(ns)
    co = _points(seed=10, n=n, dim=2)
    c = np.random.default_rng(11).normal(size=n).astype(np.float32)
    v, g = ad.vjp(builder, co, primals, c, argnums)
    assert v.shape == (n,)
    if n == 0:
        assert np.all(_flat(g) == 0.0)
        loss, g = ad.value_and_grad_sse(builder, co, primals, c, argnums)
        assert loss == 0.0 and np.all(_flat(g) == 0.0)
        return
    want, scale, value = _contraction(builder, co, primals, argnums, c)
    np.testing.assert_array_equal(v, value)
    _close(_flat(g), want, scale, "n = %d" % n)


@pytest.mark.parametrize("name", ["fam_revolutions", "fam_symmetry_rotsym"])
def test_in_place_coordinate_instruction(name, engine):
    """ROT2D rewrites its own register (a == b): the adjoint is zeroed before it accumulates."""
    fn, primals, argnums = autodiff_scenes.SCENES[name]
    builder = fn(ns)
    low, _origin = ad._lower(builder(*primals), shortcuts=False)
    from aegolius_amd import _ops
    rot = [w for w in low.code[:, 0] if _ops.OPS[int(w) & 255].name == "ROT2D"]
    assert rot and all((int(w) >> 8) & 255 == (int(w) >> 16) & 255 for w in rot)
    co = _points(seed=12)
    c = np.random.default_rng(13).normal(size=co.shape[1]).astype(np.float32)
    want, scale, _value = _contraction(builder, co, primals, argnums, c)
    for generic in (False, True):
        _v, g = ad.vjp(builder, co, primals, c, argnums, generic_rules=generic)
        _close(_flat(g), want, scale, name)


def test_resident_input_and_output_equal_the_host_path(engine):
    fn, primals, argnums = autodiff_scenes.SCENES["gradient_map_transformations"]
    builder = fn(ns)
    co, _res = ns.generate_grid((4, 4), (64, 64))
    c = np.random.default_rng(14).normal(size=65 * 65).astype(np.float32)
    v, g = ad.vjp(builder, co, primals, c, argnums)
    dco = _engine.DeviceVectorField.from_host(np.asarray(co))
    dc = _engine.DeviceField.from_host(c)
    rv, rg = ad.vjp(builder, dco, primals, dc, argnums, resident=True)
    assert isinstance(rv, _engine.DeviceField)
    np.testing.assert_array_equal(rv.numpy(), v)
    assert _flat(rg).tobytes() == _flat(g).tobytes()
    loss, gs = ad.value_and_grad_sse(builder, co, primals, c, argnums)
    rloss, rgs = ad.value_and_grad_sse(builder, dco, primals, dc, argnums)
    assert loss == rloss and _flat(gs).tobytes() == _flat(rgs).tobytes()


def test_largest_accepted_program(engine):
    """16 coordinate registers and a restore tape exactly at the limit."""
    build, _extra = largest_program()
    co = _points(seed=16)
    c = np.random.default_rng(18).normal(size=co.shape[1]).astype(np.float32)
    want, scale, value = _contraction(build, co, (0.02,), 0, c)
    v, g = ad.vjp(build, co, (0.02,), c, 0)
    np.testing.assert_array_equal(v, value)
    _close(np.array([g]), want, scale, "largest program")


def test_many_parameters_from_one_launch(engine):
    """16 circles in a union, argnums (0, 1): 32 channels (8 forward launches) against one adjoint launch."""
    rng = np.random.default_rng(19)
    primals = (rng.uniform(-1, 1, 16), rng.uniform(-1, 1, 16))
    co = _points(seed=20, dim=2)
    c = np.random.default_rng(21).normal(size=co.shape[1]).astype(np.float32)
    want, scale, _value = _contraction(_circles, co, primals, (0, 1), c)
    _v, (gx, gy) = ad.vjp(_circles, co, primals, c, (0, 1))
    assert gx.shape == (16,) and gy.shape == (16,)
    _close(np.concatenate([gx, gy]), want, scale, "16 circles")


def test_position_optimization_converges_with_sse_gradients(engine):
    """examples/autodiff/position_optimization.py with value_and_grad_sse in place of the Jacobian."""
    co, _res = ns.generate_grid((8, 8), (100, 100))
    build = autodiff_scenes.SCENES["position_optimization"][0](ns)
    target = build(2.5, -1.0).create(co).astype(np.float64)
    x = np.array([1.8, -0.4])
    _f, (jx, jy) = ad.value_and_jacfwd(build, co, (x[0], x[1]), (0, 1))
    J = np.stack([jx, jy]).astype(np.float64)
    lr = 1.0 / np.linalg.eigvalsh(2 * J.dot(J.T)).max()    # the forward-mode test's fixed step
    for _ in range(400):
        _loss, (gx, gy) = ad.value_and_grad_sse(build, co, (x[0], x[1]), target, (0, 1))
        x = x - lr * np.array([gx, gy])
        if np.linalg.norm(x - [2.5, -1.0]) < 1e-4:
            break
    assert np.linalg.norm(x - [2.5, -1.0]) < 1e-3, x


def test_multi_position_optimization_replay(engine):
    """examples/autodiff/multi_position_optimization.py: 8 x 8 at 400^2, the script's start positions and targets, Adam
    (lr 0.01) written out, the hard union as the dynamic field and the smooth-union (SMIN3, 0.75) target. The first 20
    gradients equal 2 J^T r from forward mode; after the script's 1000 iterations the best loss is below the first."""
    co, _res = ns.generate_grid((8, 8), (400, 400))
    build = autodiff_scenes.SCENES["multi_position_optimization"][0](ns)
    xt, yt = (2.2, 0.4, -2.0), (-1.0, -0.2, 1.1)
    circles = []
    for x, y in zip(xt, yt):
        c = ns.Circle(1.0)
        c.move((x, y, 0))
        circles.append(c)
    tgt = ns.CombineGeometry("SMOOTH_UNION2").combine_parametric(circles[0], circles[1], parameters=0.75)
    tgt = ns.CombineGeometry("SMOOTH_UNION2").combine_parametric(tgt, circles[2], parameters=0.75)
    target = tgt.create(co)
    params = np.array([[0.0, 0.1, -1.0], [0.0, 0.2, 0.5]])
    m, v = np.zeros_like(params), np.zeros_like(params)
    b1, b2, eps, lr = 0.9, 0.999, 1e-8, 0.01
    first = best = None
    prev = 1e16
    for it in range(1000):
        loss, (gx, gy) = ad.value_and_grad_sse(build, co, (params[0], params[1]), target, (0, 1))
        g = np.stack([gx, gy])
        if it < 20:
            f, (jx, jy) = ad.value_and_jacfwd(build, co, (params[0], params[1]), (0, 1))
            r = f.astype(np.float64) - target.astype(np.float64)
            want = 2 * np.concatenate([jx, jy]).astype(np.float64).dot(r)
            np.testing.assert_allclose(g.ravel(), want, rtol=1e-5, atol=1e-5 * np.abs(want).max())
        if first is None:
            first = best = loss
        if loss < 1e-6 or abs(loss / prev - 1) < 1e-6:
            break
        prev = loss
        best = min(best, loss)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        mh, vh = m / (1 - b1 ** (it + 1)), v / (1 - b2 ** (it + 1))
        params = params - lr * mh / (np.sqrt(vh) + eps)
    print("multi_position_optimization: %d iterations, loss %.6g -> best %.6g, params %s" % (it + 1, first, best,
                                                                                              params.tolist()))
    assert best < first
