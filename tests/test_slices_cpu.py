"""Plane stacks (aegolius_amd.slices) without a GPU: the numpy reference on hand-made stacks, Frame, the host side of
SliceStack, the lowering of a framed geometry, and every check that comes before device work."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import aegolius_amd.cores as ns  # noqa: E402
import scenes  # noqa: E402
import slices_reference as R  # noqa: E402
from aegolius_amd import _ops, slices, workloads  # noqa: E402
from aegolius_amd._lower import lower_geometry  # noqa: E402
from oracle import sdf_oracle  # noqa: E402

ENTRIES = ("sdfk_eval_grid_slices_scratch", "sdfk_eval_grid_slices", "sdfk_eval_grid_slices_finish",
           "sdfk_eval_grid_slices_measure")
AX3 = (np.array([-1.0, 0.0, 1.0]), np.array([-1.0, 0.0, 1.0]))


def _diamonds():
    F = np.ones((2, 3, 3), dtype=np.float32)
    F[:, 1, 1] = -1.0
    return F


def _oblique():
    u = np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)
    n = np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0)
    v = np.cross(n, u)
    return slices.Frame((0.1, -0.05, 0.2), u, v / np.linalg.norm(v))


# ---- the reference ----------------------------------------------------------------------------------------------------------
def test_reference_one_inside_point_per_layer():
    v, s, voff, soff = R.stack(_diamonds(), AX3, 0.0)
    assert voff.tolist() == [0, 4, 8] and soff.tolist() == [0, 4, 8]
    assert v.dtype == np.float32 and s.dtype == np.int64 and v.shape == (8, 2) and s.shape == (8, 2)
    assert s[:4].min() == 0 and s[:4].max() == 3 and s[4:].min() == 4 and s[4:].max() == 7
    np.testing.assert_array_equal(v[:4], v[4:])
    np.testing.assert_array_equal(np.sort(np.abs(v[:4]).sum(axis=1)), [0.5] * 4)       # (+-0.5, 0), (0, +-0.5)
    m = R.measures(v, s, voff, soff, AX3)
    np.testing.assert_allclose(m["area"], [0.5, 0.5], rtol=0, atol=1e-15)              # the diamond |a| + |b| <= 0.5
    np.testing.assert_allclose(m["perimeter"], [4 * np.sqrt(0.5)] * 2, rtol=1e-15)
    np.testing.assert_allclose(m["centroid"], np.zeros((2, 2)), atol=1e-15)
    assert m["segments"].tolist() == [4, 4] and m["border"].tolist() == [0, 0] and m["closed"].all()


def test_reference_open_layer():
    F = _diamonds()
    F[1] = 1.0
    F[1, 0, 1] = -1.0                                          # inside point on the border: the contour leaves the grid
    v, s, voff, soff = R.stack(F, AX3, 0.0)
    m = R.measures(v, s, voff, soff, AX3)
    assert m["closed"].tolist() == [True, False]
    assert m["border"][1] > 0 and np.isnan(m["area"][1]) and np.all(np.isnan(m["centroid"][1]))
    assert m["perimeter"][1] > 0 and m["area"][0] == 0.5
    st = slices.SliceStack(v, s, voff, soff, np.array([0.0, 1.0], np.float32), slices.Frame.axis(2),
                           [np.asarray(a, np.float32) for a in AX3])
    got = st.measures()
    np.testing.assert_array_equal(got.closed, m["closed"])
    np.testing.assert_array_equal(got.border, m["border"])
    np.testing.assert_allclose(got.area, m["area"], rtol=1e-15, equal_nan=True)
    np.testing.assert_allclose(got.perimeter, m["perimeter"], rtol=1e-15)
    assert np.isnan(got.volume())


def test_reference_holes_are_negative_area():
    F = -np.ones((1, 3, 3), dtype=np.float32)
    F[0, 1, 1] = 1.0                                           # an outside point in an inside plate: a clockwise hole
    v, s, voff, soff = R.stack(F, AX3, 0.0)
    m = R.measures(v, s, voff, soff, AX3)
    assert m["border"][0] == 0 and m["area"][0] == -0.5


# ---- Frame --------------------------------------------------------------------------------------------------------------------
def test_frame_axis_matrices_are_exact():
    want = {0: np.eye(3), 1: np.eye(3)[:, [1, 2, 0]], 2: np.eye(3)[:, [2, 0, 1]]}
    for k in range(3):
        f = slices.Frame.axis(k)
        np.testing.assert_array_equal(f.matrix, want[k])
        assert set(np.unique(f.matrix).tolist()) == {0.0, 1.0}
        np.testing.assert_array_equal(f.normal, np.eye(3)[k])
        np.testing.assert_array_equal(f.origin, np.zeros(3))
        p = f.world(0.25, 0.5, 0.75)
        assert p[k] == 0.25 and p[(k + 1) % 3] == 0.5 and p[(k + 2) % 3] == 0.75
    with pytest.raises(ValueError, match="0, 1 or 2"):
        slices.Frame.axis(3)


def test_frame_world():
    f = _oblique()
    np.testing.assert_allclose(f.normal, np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0), atol=1e-15)
    h, a, b = np.array([0.0, 0.5]), np.array([[0.1], [0.2], [0.3]]), -0.4
    got = f.world(h, a, b)
    assert got.shape == (3, 2, 3) and got.dtype == np.float64
    for i in range(3):
        for j in range(2):
            np.testing.assert_allclose(got[i, j], f.origin + h[j] * f.normal + a[i, 0] * f.u + b * f.v, atol=1e-15)


@pytest.mark.parametrize("u, v", [((1, 0, 0), (0, 2, 0)), ((1, 0, 0), (0.6, 0.8, 0)), ((1.001, 0, 0), (0, 1, 0)),
                                  ((1, 0, 0), (1, 0, 0)), ((0, 0, 0), (0, 1, 0))])
def test_frame_refuses_skewed_or_non_unit(u, v):
    with pytest.raises(ValueError, match="unit length|orthogonal"):
        slices.Frame((0, 0, 0), u, v)


def test_frame_refuses_bad_shapes():
    with pytest.raises(ValueError, match="3 finite"):
        slices.Frame((0, 0), (1, 0, 0), (0, 1, 0))
    with pytest.raises(ValueError, match="3 finite"):
        slices.Frame((0, 0, float("nan")), (1, 0, 0), (0, 1, 0))


# ---- SliceStack on the host -----------------------------------------------------------------------------------------------------
def _two_blobs_stack():
    U = np.linspace(-1, 1, 17).astype(np.float32)
    V = np.linspace(-1, 1, 21).astype(np.float32)
    H = np.array([-0.1, 0.0, 0.3], dtype=np.float32)
    a, b = np.meshgrid(U.astype(np.float64), V.astype(np.float64), indexing="ij")
    F = np.empty((3, U.size, V.size), dtype=np.float32)
    F[0] = np.hypot(a + 0.4, b) - 0.3                                                  # one disc
    F[1] = np.minimum(np.hypot(a + 0.4, b) - 0.3, np.hypot(a - 0.45, b - 0.2) - 0.25)  # two discs
    F[2] = np.abs(np.hypot(a, b) - 0.5) - 0.2                                          # a ring: outer loop and hole
    v, s, voff, soff = R.stack(F, (U, V), 0.0)
    return slices.SliceStack(v, s, voff, soff, H, slices.Frame.axis(2), (U, V)), F


def test_layer_rebases_ids_and_loops_close():
    st, F = _two_blobs_stack()
    assert len(st) == 3
    import mesh_reference
    for l, loops in enumerate((1, 2, 2)):
        c = st.layer(l)
        wv, ws = mesh_reference.extract(F[l], st.axes, 0.0)
        np.testing.assert_array_equal(c.vertices.view(np.uint32), wv.view(np.uint32))
        np.testing.assert_array_equal(c.segments, ws)
        assert c.segments.min() == 0 and c.segments.max() == len(c.vertices) - 1
        got = c.loops()
        assert len(got) == loops and all(lp[0] == lp[-1] for lp in got)
    np.testing.assert_array_equal(st.layer(-1).segments, st.layer(2).segments)
    with pytest.raises(IndexError):
        st.layer(3)
    m = st.measures()
    assert m.closed.all()
    assert abs(m.area[0] - np.pi * 0.09) < 0.02 and abs(m.area[2] - np.pi * (0.49 - 0.09)) < 0.05
    assert abs(m.centroid[0, 0] + 0.4) < 0.01 and abs(m.centroid[0, 1]) < 0.01
    want = 0.5 * (m.area[0] + m.area[1]) * (0.0 - -0.1) + 0.5 * (m.area[1] + m.area[2]) * (np.float32(0.3) - 0.0)
    np.testing.assert_allclose(m.volume(), want, rtol=1e-6)


def test_world_vertices():
    st, _ = _two_blobs_stack()
    w = st.world_vertices()
    assert w.shape == (len(st.vertices), 3) and w.dtype == np.float64
    for l in range(3):
        sl = slice(st.vertex_offsets[l], st.vertex_offsets[l + 1])
        np.testing.assert_array_equal(w[sl, 2], np.full(sl.stop - sl.start, np.float64(st.heights[l])))
        np.testing.assert_array_equal(w[sl, :2], st.vertices[sl].astype(np.float64))
    st.frame = _oblique()
    w = st.world_vertices()
    np.testing.assert_allclose((w - st.frame.origin).dot(st.frame.normal),
                               np.repeat(st.heights.astype(np.float64), np.diff(st.vertex_offsets)), atol=1e-12)


def test_svg_has_one_path_per_loop(tmp_path):
    st, _ = _two_blobs_stack()
    for l, loops in enumerate((1, 2, 2)):
        path = tmp_path / ("layer%d.svg" % l)
        st.write_svg(str(path), l)
        text = path.read_text()
        assert text.startswith("<svg") and text.count("<path ") == loops and text.count(" Z\"") == loops


# ---- the framed geometry ------------------------------------------------------------------------------------------------------
def _rotated_box():
    b = ns.Box(0.5, 0.4, 0.3)
    b.rotate(0.4, (0, 1, 1))
    b.move((0.1, -0.05, 0.02))
    return b


@pytest.mark.parametrize("scene", ["sphere", "box", "cfg2", "cfg5"])
def test_axis0_lowers_to_the_geometrys_own_program(scene):
    g = {"sphere": lambda: ns.Sphere(0.5), "box": _rotated_box, "cfg2": lambda: workloads.cfg2_tree(ns),
         "cfg5": lambda: workloads.cfg5_tree(ns)}[scene]()
    assert lower_geometry(slices.Frame.axis(0).apply(g)).key() == lower_geometry(g).key()


def test_frame_is_one_outer_xform_never_composed():
    g = _rotated_box()
    own = lower_geometry(g)
    for frame in (slices.Frame.axis(1), slices.Frame.axis(2), _oblique()):
        low = lower_geometry(frame.apply(g))
        assert len(low.code) == len(own.code) + 1
        assert _ops.OPS[int(low.code[0][0]) & 255].name == "XFORM"
        np.testing.assert_array_equal(low.params[:9], frame.matrix.ravel().astype(np.float32))
        np.testing.assert_array_equal(low.params[9:12], (-frame.origin).astype(np.float32))
        np.testing.assert_array_equal(low.params[12:], own.params)                      # the inner program's constants
        assert [_ops.OPS[int(w) & 255].name for w, _ in low.code[1:]] == [_ops.OPS[int(w) & 255].name for w, _ in own.code]


def test_apply_leaves_the_geometry_untouched():
    g = _rotated_box()
    before = (lower_geometry(g).key(), g.rotation_matrix.copy(), g.center.copy(), g.scale)
    framed = _oblique().apply(g)
    assert framed is not g and framed.inner is g
    assert lower_geometry(g).key() == before[0]
    np.testing.assert_array_equal(g.rotation_matrix, before[1])
    np.testing.assert_array_equal(g.center, before[2])
    framed.move((0.5, 0, 0))                                   # an ordinary node from then on
    assert framed.frame_map is None
    with pytest.raises(TypeError, match="geometry"):
        _oblique().apply(np.zeros(8))


@pytest.mark.parametrize("scene", ["sphere", "box", "cfg2"])
def test_axis2_create_is_the_geometry_at_the_permuted_points(scene):
    g = {"sphere": lambda: ns.Sphere(0.5), "box": _rotated_box, "cfg2": lambda: workloads.cfg2_tree(ns)}[scene]()
    rng = np.random.default_rng(3)
    co = rng.uniform(-1, 1, (3, 500))                          # (h, a, b)
    got = sdf_oracle.evaluate(slices.Frame.axis(2).apply(g), co)
    np.testing.assert_array_equal(got, sdf_oracle.evaluate(g, co[[1, 2, 0]]))           # (x, y, z) = (a, b, h)
    got = sdf_oracle.evaluate(slices.Frame.axis(1).apply(g), co)
    np.testing.assert_array_equal(got, sdf_oracle.evaluate(g, co[[2, 0, 1]]))           # (x, y, z) = (b, h, a)
    f = _oblique()
    got = sdf_oracle.evaluate(f.apply(g), co)
    np.testing.assert_allclose(got, sdf_oracle.evaluate(g, f.world(co[0], co[1], co[2]).T), rtol=0, atol=1e-13)


# ---- refusals before device work ---------------------------------------------------------------------------------------------
def test_staged_trees_are_refused_by_operator_name():
    build, key = scenes.GRID_SCENES["grid_conv_sphere_3x3x3"]
    _, res = scenes.GRIDS[key]
    ax = np.linspace(-1, 1, 9)
    with pytest.raises(ValueError, match="conv_averaging"):
        slices.stack(build(ns, res), (ax, ax), ax)
    with pytest.raises(ValueError, match="conv_averaging"):
        slices.measures(build(ns, res), (ax, ax), ax, normal=0)


def test_validation_errors():
    g = ns.Sphere(0.5)
    ax = np.linspace(-1, 1, 9)
    for fn in (slices.stack, slices.measures):
        with pytest.raises(ValueError, match="NaN"):
            fn(g, (ax, ax), ax, level=float("nan"))
        with pytest.raises(ValueError, match="heights is not strictly increasing"):
            fn(g, (ax, ax), ax[::-1])
        with pytest.raises(ValueError, match="axis U is not strictly increasing"):
            fn(g, (np.r_[ax[:4], ax[3:]], ax), ax)
        with pytest.raises(ValueError, match="axis V is not strictly increasing"):
            fn(g, (ax, np.array([0.0, 1.0, 1.0 + 1e-12])), ax)           # equal as float32
        with pytest.raises(ValueError, match="axis U has 1 point"):
            fn(g, (ax[:1], ax), ax)
        with pytest.raises(ValueError, match="axis V has 1 point"):
            fn(g, (ax, ax[:1]), ax)
        with pytest.raises(ValueError, match="heights has 0 point"):
            fn(g, (ax, ax), [])
        with pytest.raises(ValueError, match="two in-plane tables"):
            fn(g, (ax, ax, ax), ax)
        with pytest.raises(ValueError, match="normal"):
            fn(g, (ax, ax), ax, normal=3)
        with pytest.raises(TypeError, match="fields are not sliced"):
            fn(np.zeros(9 ** 3), (ax, ax), ax)
    with pytest.raises(ValueError, match="NaN"):
        slices.from_geometry(g, (2, 2, 2), (9, 9, 9), level=float("nan"))
    with pytest.raises(ValueError, match="3 entries"):
        slices.from_geometry(g, (2, 2), (9, 9))


def test_entries_are_declared_and_exported(built):
    header = open(os.path.join(os.path.dirname(HERE), "include", "sdfk.h")).read()
    for name in ENTRIES:
        assert name in built.SIGNATURES and hasattr(built.lib(), name)
        assert name + "(" in header


@pytest.mark.parametrize("shape", [(1025, 1025, 1025), (1, 2, 2), (257, 257, 257), (3, 5, 7), (9, 40, 48), (1, 4097, 4097)])
def test_scratch_is_at_most_one_byte_per_point(built, shape):
    n = int(np.prod(shape, dtype=np.int64))
    got = built.lib().sdfk_eval_grid_slices_scratch(*shape)
    assert got <= n + (1 << 20) + 16 * (shape[0] + 1)
    assert got >= built.lib().sdfk_field_isosurface_scratch(*shape) + 16 * (shape[0] + 1)


def test_abi_refuses_bad_calls_without_touching_the_device(built):
    import ctypes
    L = built.lib()
    t = np.ascontiguousarray(np.linspace(-1, 1, 5), dtype=np.float32)
    nv, ns_ = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = L.sdfk_eval_grid_slices(None, built._ptr(t), 5, built._ptr(t), 5, built._ptr(t), 5, 0.0, ctypes.byref(nv),
                                 ctypes.byref(ns_), ctypes.c_void_p(4096), None, 0)
    assert rc != 0 and "null program" in built.last_error()
    off = np.zeros(6, dtype=np.int64)
    rc = L.sdfk_eval_grid_slices_finish(None, 5, 5, 5, 0.0, 0, 0, None, 0, None, 0, 4, built._ptr(off), built._ptr(off),
                                        ctypes.c_void_p(4096), None, 0)
    assert rc != 0
    out = np.zeros(30)
    rc = L.sdfk_eval_grid_slices_measure(None, built._ptr(t), 5, built._ptr(t), 5, built._ptr(t), 5, 0.0, built._ptr(out),
                                         built._ptr(off), built._ptr(off), ctypes.c_void_p(4096), None, 0)
    assert rc != 0


def test_no_gpu_means_an_error_not_a_fallback(built):
    ax = np.linspace(-1, 1, 9)
    if built.device_count() > 0:
        assert len(slices.stack(ns.Sphere(0.5), (ax, ax), ax).vertices) > 0
    else:
        with pytest.raises(built.SdfkError, match="no HIP device"):
            slices.stack(ns.Sphere(0.5), (ax, ax), ax)
