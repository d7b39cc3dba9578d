"""aegolius_amd.redistance on the GPU (kernels: csrc/sdfk_redistance.inc): equal, bit for bit, to the numpy reference
(tests/redistance_reference.py) on the package's own create() fields, for both near modes; bands; fields without a
crossing, with NaN points, other levels, crossings at grid points; resident and geometry inputs; run to run; the C entry
with exactly the scratch it asks for.

The shapes are the smallest that reach: the smallest grid, odd sizes, lines that are no multiple of a wave and a z line over
two waves (the LDS kernel; z lines of at most 64 points take the strided one), a contiguous line longer than one staging
window of 1024 points, 2-D (where y is the contiguous axis), non-uniform tables."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import aegolius_amd.cores as ns  # noqa: E402
import redistance_reference as ref  # noqa: E402
from aegolius_amd import _engine, redistance  # noqa: E402
from aegolius_amd._eval import config  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32

CASES = [(s, g) for g in ref.GRIDS for s in ref.scenes_for(g)]
BAND_GRIDS = ["17x13x11", "5x67x130", "3x3x1100", "9x11x13nu", "33x29", "3x130"]


@functools.lru_cache(maxsize=None)
def field_of(scene, grid):
    """The package's own field of the scene on the grid: create() on the grid's coordinates."""
    f = np.asarray(ref.build(scene, grid).create(ref.coords(ref.GRIDS[grid])), dtype=F32)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def q_of(scene, grid, level=0.0):
    q = ref.separable(field_of(scene, grid), ref.GRIDS[grid], level)
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def want_of(scene, grid, near, level=0.0):
    out = ref.finish(q_of(scene, grid, level), field_of(scene, grid), ref.GRIDS[grid], level, None, near)
    out.setflags(write=False)
    return out


def same_bits(got, want):
    got = np.asarray(got)
    assert got.dtype == F32 and got.shape == want.shape
    diff = np.flatnonzero(ref.bits(got) != ref.bits(want))
    assert diff.size == 0, "%d of %d differ, first at %d: %r != %r" % (diff.size, want.size, diff[0], got[diff[0]], want[diff[0]])


def min_step(axes):
    return min(float(np.diff(np.asarray(a, dtype=np.float64).astype(F32)).min()) for a in axes)


def cut(free, band):
    return np.copysign(np.minimum(np.abs(free), F32(band)), free).astype(F32)


# ---- bit-equality -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("near", redistance.NEAR)
@pytest.mark.parametrize("scene,grid", CASES)
def test_equals_the_reference_bit_for_bit(scene, grid, near):
    f = field_of(scene, grid)
    stats = {}
    got = redistance.redistance(f, ref.GRIDS[grid], near=near, stats=stats)
    same_bits(got, want_of(scene, grid, near))
    assert stats["seeds"] == ref.seed_count(f, ref.GRIDS[grid])
    names = redistance.PASSES_2D if len(ref.GRIDS[grid]) == 2 else redistance.PASSES_3D
    assert tuple(stats["ms"]) == names and all(v >= 0.0 for v in stats["ms"].values())
    if scene == "smooth_union" and grid != "2x2x2":
        assert stats["seeds"] > 0                               # the case is not an empty one


@pytest.mark.parametrize("which", ["half", "three", "beyond"])
@pytest.mark.parametrize("near", redistance.NEAR)
@pytest.mark.parametrize("grid", BAND_GRIDS)
def test_band_is_the_cut_of_the_unbounded_result(grid, near, which):
    axes = ref.GRIDS[grid]
    diagonal = float(np.sqrt(sum((a[-1] - a[0]) ** 2 for a in axes)))
    band = {"half": 0.5 * min_step(axes), "three": 3.0 * min_step(axes), "beyond": 1.5 * diagonal}[which]
    for scene in ("smooth_union", "twist_bend" if len(axes) == 3 else "sign"):
        got = redistance.redistance(field_of(scene, grid), axes, band=band, near=near)
        same_bits(got, cut(want_of(scene, grid, near), band))


# ---- edge cases -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["17x13x11", "3x130", "5x67x130"])
def test_no_crossing_gives_infinity_or_the_band(grid):
    axes = ref.GRIDS[grid]
    f = np.abs(field_of("smooth_union", grid)) + F32(0.5)
    stats = {}
    assert np.all(np.isposinf(redistance.redistance(f, axes, stats=stats))) and stats["seeds"] == 0
    assert np.all(np.isneginf(redistance.redistance(-f, axes)))
    same_bits(redistance.redistance(f, axes, band=0.25), np.full(f.size, 0.25, F32))
    same_bits(redistance.redistance(-f, axes, band=0.25, near="seeds"), np.full(f.size, -0.25, F32))


@pytest.mark.parametrize("near", redistance.NEAR)
@pytest.mark.parametrize("grid", ["17x13x11", "5x67x130", "33x29"])
def test_nan_points_put_the_seed_at_the_other_end_and_come_out_positive(grid, near):
    axes = ref.GRIDS[grid]
    f = field_of("smooth_union", grid).copy()
    f[::7] = np.nan
    f[100:130] = np.nan
    got = redistance.redistance(f, axes, near=near)
    same_bits(got, ref.redistance(f, axes, near=near))
    assert np.all(got[np.isnan(f)] >= 0) and not np.signbit(got[np.isnan(f)]).any() and not np.isnan(got).any()


@pytest.mark.parametrize("level", [0.05, -0.1])
@pytest.mark.parametrize("grid", ["17x13x11", "9x11x13nu", "33x29"])
def test_other_levels(grid, level):
    axes = ref.GRIDS[grid]
    for near in redistance.NEAR:
        stats = {}
        got = redistance.redistance(field_of("smooth_union", grid), axes, level=level, near=near, stats=stats)
        same_bits(got, ref.finish(q_of("smooth_union", grid, level), field_of("smooth_union", grid), axes, level, None, near))
        assert stats["seeds"] == ref.seed_count(field_of("smooth_union", grid), axes, level) > 0


@pytest.mark.parametrize("grid", ["17x13x11", "5x67x130", "3x130"])
def test_crossings_exactly_at_grid_points(grid):
    """An integer-valued field: f == level on whole planes of grid points, t = 0 or 1 on their edges."""
    axes = ref.GRIDS[grid]
    idx = np.meshgrid(*[np.arange(len(a)) for a in axes], indexing="ij")
    f = (sum(idx) - sum(len(a) for a in axes) // 3).astype(F32).ravel()
    for level in (0.0, 2.0):
        for near in redistance.NEAR:
            got = redistance.redistance(f, axes, level=level, near=near)
            same_bits(got, ref.redistance(f, axes, level, near=near))
            assert np.all(got[f == level] == 0) and np.signbit(got[f == level]).all()     # on the level set: -0.0


# ---- input kinds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["17x13x11", "33x29"])
def test_resident_input_and_output(grid):
    axes = ref.GRIDS[grid]
    f = field_of("smooth_union", grid)
    want = want_of("smooth_union", grid, "gradient")
    with _engine.DeviceField.from_host(f, config.device) as dev:
        same_bits(redistance.redistance(dev, axes), want)
        out = redistance.redistance(dev, axes, resident=True)
        try:
            assert isinstance(out, _engine.DeviceField) and out.n == f.size and out.ptr != dev.ptr
            same_bits(out.numpy(), want)
            same_bits(redistance.redistance(out, axes, near="seeds", band=0.2),      # a result is a field like any other
                      ref.redistance(want, axes, band=0.2, near="seeds"))
        finally:
            out.free()
        same_bits(dev.numpy(), f)                               # the input is unchanged
    out = redistance.redistance(f, axes, resident=True)
    try:
        same_bits(out.numpy(), want)
    finally:
        out.free()


def test_geometry_input_equals_create_plus_field():
    axes = ref.GRIDS["17x13x11"]
    want = redistance.redistance(field_of("twist_bend", "17x13x11"), axes, band=0.3)
    same_bits(redistance.redistance(ref.build("twist_bend", "17x13x11"), axes, band=0.3), want)
    same_bits(redistance.redistance(ref.build("smooth_union", "33x29"), ref.GRIDS["33x29"]),
              want_of("smooth_union", "33x29", "gradient"))
    grid, _ = ns.generate_grid((2, 2, 2), (17, 13, 11))         # the same tables, as a tagged array
    same_bits(redistance.redistance(ref.build("twist_bend", "17x13x11"), grid, band=0.3), want)
    same_bits(redistance.from_geometry(ref.build("twist_bend", "17x13x11"), (2, 2, 2), (17, 13, 11), band=0.3), want)
    flat, _ = ns.generate_grid((2, 2), (33, 29))
    same_bits(redistance.from_geometry(ref.build("smooth_union", "33x29"), (2, 2), (33, 29), near="seeds"),
              redistance.redistance(ref.build("smooth_union", "33x29").create(flat), flat, near="seeds"))


def test_staged_geometry_input():
    def shell():
        s = ns.Sphere(0.62)
        s.boundary()
        s.signed((17, 17, 17))
        return s
    grid, _ = ns.generate_grid((2, 2, 2), (17, 17, 17))
    f = np.asarray(shell().create(grid), dtype=F32)
    want = ref.redistance(f, grid.grid_axes)
    assert ref.seed_count(f, grid.grid_axes) > 0
    same_bits(redistance.redistance(f, grid), want)
    same_bits(redistance.redistance(shell(), grid), want)
    same_bits(redistance.from_geometry(shell(), (2, 2, 2), (17, 17, 17)), want)
    out = redistance.redistance(shell(), grid, resident=True)
    try:
        same_bits(out.numpy(), want)
    finally:
        out.free()


# ---- run to run -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["5x67x130", "3x3x1100", "33x29"])
def test_two_runs_give_the_same_bits_and_count_the_seeds(grid):
    axes = ref.GRIDS[grid]
    f = field_of("smooth_union", grid)
    a, b = {}, {}
    first = redistance.redistance(f, axes, stats=a)
    second = redistance.redistance(f, axes, stats=b)
    same_bits(first, second)
    assert a["seeds"] == b["seeds"] == ref.seed_count(f, axes) > 0


# ---- the C entry ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["17x13x11", "3x3x1100", "33x29"])
def test_c_entry_stays_inside_its_scratch_and_output(grid):
    L = _engine.lib()
    axes = ref.GRIDS[grid]
    tabs = ref.tables(axes) + ([np.zeros(1, F32)] if len(axes) == 2 else [])
    shape = [t.size for t in tabs]
    n = int(np.prod(shape))
    f = field_of("smooth_union", grid)
    need = L.sdfk_field_redistance_scratch(*shape)
    assert need == 8 * n
    guard = np.arange(1024, dtype=np.uint32) * np.uint32(2654435761)
    _, tab = _engine.axis_args(tabs)
    seeds = ctypes.c_int64(-1)
    ms = (ctypes.c_float * 9)()
    with _engine.DeviceField.from_host(f, config.device) as dev, \
            _engine.DeviceBuffer(need + guard.nbytes, config.device, "scratch + guard") as scratch, \
            _engine.DeviceBuffer(4 * n + guard.nbytes, config.device, "output + guard") as out:
        scratch.upload(guard, need)
        out.upload(guard, 4 * n)
        _engine.check(L.sdfk_field_redistance(ctypes.c_void_p(dev.ptr), *tab, 0.0, 0.0, 1, out.at(0, 4 * n), scratch.at(0, need),
                                              ctypes.byref(seeds), ms, None), "sdfk_field_redistance")
        same_bits(out.download(np.empty(n, F32)), want_of("smooth_union", grid, "gradient"))
        assert np.array_equal(scratch.download(np.empty_like(guard), need), guard)
        assert np.array_equal(out.download(np.empty_like(guard), 4 * n), guard)
        same_bits(dev.numpy(), f)
        assert seeds.value == ref.seed_count(f, axes)
        # a refusal launches nothing and says why
        assert L.sdfk_field_redistance(ctypes.c_void_p(dev.ptr), *tab, 0.0, 0.0, 1, ctypes.c_void_p(dev.ptr), scratch.at(),
                                       ctypes.byref(seeds), None, None) == -1
        assert "must not be the field" in _engine.last_error()
