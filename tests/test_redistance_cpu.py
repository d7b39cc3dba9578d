"""aegolius_amd.redistance without a GPU: the numpy reference against itself (brute force = separable passes, bit for bit),
its seeds against tests/mesh_reference.py, a closed form, a soundness bound, every refusal of the public functions, and
the new entry points."""
import os

import numpy as np
import pytest

import aegolius_amd.cores as ns
import mesh_reference
import redistance_reference as ref
from aegolius_amd import redistance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _grid(axes):
    ax = [np.asarray(a, dtype=np.float64).astype(F32) for a in axes]
    return np.meshgrid(*ax, indexing="ij")


def _radius(axes, centre=(0.07, -0.04, 0.11)):
    g = _grid(axes)
    return np.sqrt(sum((x - F32(c)) * (x - F32(c)) for x, c in zip(g, centre))).astype(F32)


def _scaled_sphere(axes):
    return (F32(3.0) * (_radius(axes) - F32(0.6))).ravel()


def _squared_sphere(axes):
    r = _radius(axes)
    return (r * r - F32(0.36)).ravel()


def _sign_field(axes):
    return np.sign(_scaled_sphere(axes)).astype(F32)


def _with_nans(axes):
    f = _squared_sphere(axes).copy()
    f[::7] = np.nan
    return f


def _at_grid_points(axes):
    """Integer-valued: crossings exactly at grid points (f == level) on whole planes."""
    g = _grid(axes)
    idx = [np.searchsorted(np.asarray(a, dtype=np.float64).astype(F32), x) for a, x in zip(axes, g)]
    return (sum(idx) - (sum(len(a) for a in axes) // 3)).astype(F32).ravel()


def _waves(axes):
    g = _grid(axes)
    return sum(np.sin(F32(3.0 + k) * x + F32(k)) for k, x in enumerate(g)).astype(F32).ravel()


FIELDS = {"3(r-R)": _scaled_sphere, "r^2-R^2": _squared_sphere, "sign": _sign_field, "nan": _with_nans,
          "grid_points": _at_grid_points, "waves": _waves}
CPU_GRIDS = ["2x2x2", "17x13x11", "9x11x13nu", "33x29", "3x130"]


@pytest.mark.parametrize("grid", CPU_GRIDS)
@pytest.mark.parametrize("field", list(FIELDS))
@pytest.mark.parametrize("level", [0.0, 0.25])
def test_brute_force_equals_the_separable_passes_bit_for_bit(grid, field, level):
    axes = ref.GRIDS[grid]
    f = FIELDS[field](axes)
    a, b = ref.brute(f, axes, level), ref.separable(f, axes, level)
    assert a.dtype == b.dtype == F32 and np.array_equal(ref.bits(a), ref.bits(b))
    assert not np.isnan(a).any() and (a >= 0).all()
    for near in redistance.NEAR:
        out = ref.redistance(f, axes, level, near=near)
        assert np.array_equal(ref.bits(out), ref.bits(ref.redistance(f, axes, level, near=near, method=ref.brute)))
        assert np.array_equal(out < 0, ref.inside(f, level) & (np.abs(out) > 0))          # the sign is the inside test
        assert not np.isnan(out).any()


def test_a_long_line_and_many_seeds_agree_as_well():
    axes = ref.GRIDS["5x67x130"]
    f = _waves(axes)
    assert np.array_equal(ref.bits(ref.brute(f, axes)), ref.bits(ref.separable(f, axes)))


@pytest.mark.parametrize("grid", CPU_GRIDS)
@pytest.mark.parametrize("field", ["r^2-R^2", "nan", "grid_points", "sign"])
def test_seeds_are_the_vertices_of_the_mesh(grid, field):
    axes = ref.GRIDS[grid]
    f = FIELDS[field](axes)
    for level in (0.0, 0.25):
        verts, _ = mesh_reference.extract(f, axes, level)
        pts = ref.seed_points(f, axes, level)
        assert pts.shape == verts.shape and ref.seed_count(f, axes, level) == len(verts)
        as_set = lambda v: sorted(map(bytes, np.ascontiguousarray(v, dtype=F32)))      # noqa: E731
        assert as_set(pts) == as_set(verts)


@pytest.mark.parametrize("near", redistance.NEAR)
def test_closed_form_of_a_plane_on_a_nonuniform_grid(near):
    axes = ref.nonuniform((23, 7, 9), seed=11)
    x = _grid(axes)[0]
    c = 0.5 * (axes[0][9] + axes[0][10]) + 0.013                      # between two grid points
    f = (F32(3.0) * (x - F32(c))).ravel()
    out = ref.redistance(f, axes, near=near).astype(np.float64)
    want = (x.astype(np.float64) - float(F32(c))).ravel()
    assert np.all(np.abs(out - want) <= 1e-6 * np.maximum(1.0, np.abs(want)))


@pytest.mark.parametrize("near", redistance.NEAR)
def test_coarse_soundness_on_an_exact_sphere(near):
    """Every seed lies on a grid edge that the true surface crosses too, so a seed is within one cell diagonal of the
    surface and the surface within one of a seed: | |ref| - |true| | <= 2 sqrt(3) h."""
    axes = ref.box((17, 17, 17))
    h = 2.0 / 16
    true = (_radius(axes, (0, 0, 0)) - F32(0.6)).ravel()
    out = ref.redistance(true, axes, near=near)
    assert np.all(np.abs(np.abs(out.astype(np.float64)) - np.abs(true.astype(np.float64))) <= 2 * np.sqrt(3) * h)
    assert np.array_equal(out <= 0, true <= 0)


def test_band_and_empty_fields_in_the_reference():
    axes = ref.GRIDS["17x13x11"]
    f = _squared_sphere(axes)
    free = ref.redistance(f, axes, near="seeds")
    cut = ref.redistance(f, axes, band=0.3, near="seeds")
    assert np.array_equal(ref.bits(cut), ref.bits(np.copysign(np.minimum(np.abs(free), F32(0.3)), free)))
    none = ref.redistance(np.abs(f) + F32(1), axes)
    assert np.all(np.isposinf(none))
    assert np.all(ref.redistance(-np.abs(f) - F32(1), axes, band=0.5) == F32(-0.5))


# ---- the public functions refuse before they need a GPU ---------------------------------------------------------------
AXES = ref.GRIDS["17x13x11"]
N = 17 * 13 * 11


@pytest.mark.parametrize("band", [0, 0.0, -1.0, float("nan"), float("inf"), -float("inf")])
def test_band_must_be_finite_and_positive(band):
    with pytest.raises(ValueError, match="band"):
        redistance.redistance(np.zeros(N, F32), AXES, band=band)
    with pytest.raises(ValueError, match="band"):
        redistance.from_geometry(ns.Sphere(0.3), (2, 2, 2), (9, 9, 9), band=band)


def test_unknown_near_mode():
    with pytest.raises(ValueError, match="near"):
        redistance.redistance(np.zeros(N, F32), AXES, near="both")
    with pytest.raises(ValueError, match="near"):
        redistance.from_geometry(ns.Sphere(0.3), (2, 2, 2), (9, 9, 9), near=None)


def test_field_size_must_match_the_axes():
    with pytest.raises(ValueError, match="the axes span 17x13x11"):
        redistance.redistance(np.zeros(N - 1, F32), AXES)
    with pytest.raises(ValueError, match="the axes span 33x29"):
        redistance.redistance(np.zeros(N, F32), ref.GRIDS["33x29"])


def test_untagged_grid_array_and_bad_tables_are_refused():
    grid, _ = ns.generate_grid((2, 2, 2), (5, 5, 5))
    with pytest.raises(ValueError, match="no longer tagged"):
        redistance.redistance(np.zeros(125, F32), np.array(grid))
    with pytest.raises(ValueError, match="strictly increasing"):
        redistance.redistance(np.zeros(27, F32), [np.array([0.0, 1.0, 1.0])] * 3)
    with pytest.raises(ValueError, match="at least 2"):
        redistance.redistance(np.zeros(9, F32), [np.arange(3.0), np.arange(3.0), np.array([5.0])])
    with pytest.raises(ValueError, match="axis tables"):
        redistance.redistance(np.zeros(3, F32), [np.arange(3.0)])


def test_nan_level_is_refused():
    with pytest.raises(ValueError, match="level is NaN"):
        redistance.redistance(np.zeros(N, F32), AXES, level=float("nan"))
    with pytest.raises(ValueError, match="level is NaN"):
        redistance.from_geometry(ns.Sphere(0.3), (2, 2, 2), (9, 9, 9), level=float("nan"))


def test_from_geometry_takes_two_or_three_sizes_and_a_geometry():
    with pytest.raises(ValueError, match="2 or 3"):
        redistance.from_geometry(ns.Sphere(0.3), (2,), (9,))
    with pytest.raises(ValueError, match="geometry"):
        redistance.from_geometry(np.zeros(729, F32), (2, 2, 2), (9, 9, 9))


def test_axes_of_a_2d_generate_grid_are_taken_as_two():
    grid, _ = ns.generate_grid((2, 2), (9, 7))
    tabs = redistance._axes(grid)
    assert [t.size for t in tabs] == [9, 7] and all(t.dtype == F32 for t in tabs)
    assert [t.size for t in redistance._axes(ref.GRIDS["33x29"])] == [33, 29]
    assert [t.size for t in redistance._axes(AXES)] == [17, 13, 11]


def test_entry_points_are_declared_bound_and_exported(built):
    import aegolius_amd
    assert aegolius_amd.redistance is redistance
    header = open(os.path.join(ROOT, "include", "sdfk.h")).read()
    for name in ("sdfk_field_redistance_scratch", "sdfk_field_redistance"):
        assert name in built.SIGNATURES and hasattr(built.lib(), name) and name + "(" in header
    lib = built.lib()
    assert lib.sdfk_abi_version() == 1
    assert lib.sdfk_field_redistance_scratch(17, 13, 11) == 2 * 4 * N           # exactly 2 N floats
    assert lib.sdfk_field_redistance_scratch(33, 29, 1) == 2 * 4 * 33 * 29
    assert "SDFK_REDISTANCE_PASSES %d" % len(redistance.PASSES_3D) in header


def test_c_entry_validates_on_the_host(built):
    """Refusals of the C entry that need no device: they return -1 before anything is launched."""
    import ctypes
    lib = built.lib()
    ax = np.linspace(-1, 1, 5).astype(F32)
    bad = np.array([0, 1, 1, 2, 3], dtype=F32)
    seeds = ctypes.c_int64(0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                      # noqa: E731
    fake, fake2, fake3 = ctypes.c_void_p(256), ctypes.c_void_p(512), ctypes.c_void_p(1024)

    def call(field=fake, a0=ax, n0=5, a2=ax, n2=5, level=0.0, band=0.0, near=1, out=fake2, scratch=fake3, count=seeds):
        return lib.sdfk_field_redistance(field, p(a0), n0, p(ax), 5, p(a2), n2, level, band, near, out, scratch,
                                         ctypes.byref(count) if count is not None else None, None, None)
    for kwargs, text in (({"field": None}, "null"), ({"out": fake}, "must not be the field"), ({"n0": 1}, "2 to 2^31"),
                         ({"level": float("nan")}, "level is NaN"), ({"band": float("inf")}, "band"),
                         ({"band": float("nan")}, "band"), ({"near": 2}, "near"), ({"count": None}, "seed counter"),
                         ({"a0": bad}, "strictly increasing"), ({"scratch": None}, "null")):
        assert call(**kwargs) == -1, kwargs
        assert text in built.last_error(), (kwargs, built.last_error())
