"""aegolius_amd.moments on the GPU (kernels: csrc/sdfk_moments.inc, csrc/sdfk_momdev.h): the integer moments equal, bit for
bit, the numpy sums over the package's own field on the fine grid; the same under every mode, slab size and run; the same
classification as occupancy; the float64 oracle; closed forms. Definition: tests/moments_reference.py; lattice, scenes and
grids: tests/occupancy_reference.py.

The shapes are the smallest that reach: K = 1, 8, 16, 64 and 512 (both lane layouts and eight rounds per cell), entry counts
that do not fill the last wave (8 and 105 cells), rows longer than a wave (67, 130), entries of one wave in different rows
and planes, and slab seams."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import aegolius_amd.cores as ns  # noqa: E402
import moments_reference as mref  # noqa: E402
import occupancy_reference as ref  # noqa: E402
from aegolius_amd import _engine, moments, occupancy  # noqa: E402
from aegolius_amd._eval import config, program_for  # noqa: E402
from aegolius_amd._lower import lower_geometry  # noqa: E402

pytestmark = pytest.mark.gpu

SCENES_3D = ("cfg1", "cfg2", "cfg5", "sheared", "union300", "cfg3")        # cfg3: no bound, so nothing is skipped
COMBOS = [("2^3", 1, 0.0), ("2^3", 4, 0.05), ("2^3", 8, 0.0), ("3x5x7", 2, 0.05), ("3x5x7", 4, 0.0), ("17^3", 1, 0.0),
          ("17^3", 2, -0.03), ("17^3", 4, 0.0), ("5x5x67", 4, -0.03), ("5x5x67", 8, 0.0), ("33x31x64", 2, 0.05),
          ("33x31x64", 1, 0.0)]
COMBOS_2D = [("65x63", 1, -0.03), ("65x63", 2, 0.0), ("65x63", 4, 0.05), ("65x63", 8, 0.0), ("3x130", 2, 0.05), ("3x130", 4, 0.0),
             ("3x130", 8, 0.0)]
CASES = [(s, g, k, lv) for s in SCENES_3D for g, k, lv in COMBOS] + [("cfg4", g, k, lv) for g, k, lv in COMBOS_2D]


class mode:
    def __init__(self, m):
        self.m = m

    def __enter__(self):
        self.old, config.mode = config.mode, self.m

    def __exit__(self, *exc):
        config.mode = self.old


@functools.lru_cache(maxsize=None)
def fine_moments(scene, grid, k, level):
    """M from the package's existing path, as test_gpu_occupancy.fine_counts makes its field: Program.eval_grid of the
    fine grid the reference's tables span, downloaded, compared with the level, summed by the reference."""
    axes = ref.grid_for(scene, grid)
    tabs = ref.tables(axes, k)
    n = int(np.prod([t.size for t in tabs]))
    prog = program_for(lower_geometry(ref.build(scene)))
    with _engine.DeviceField(n, config.device) as field:
        prog.eval_grid(tabs, 0, n, field.ptr, mode=config.mode)
        _engine.check(_engine.lib().sdfk_sync(None), "sdfk_sync")
        values = field.numpy()
    with np.errstate(invalid="ignore"):
        return mref.lattice_moments(values <= np.float32(level), axes, k)


def run(scene, grid, k, level, **kw):
    return moments.moments(ref.build(scene), ref.grid_for(scene, grid), k, level, **kw)


# ---- 1. equal to numpy on the fine field, bit for bit ---------------------------------------------------------------------
@pytest.mark.parametrize("scene,grid,k,level", CASES)
def test_equal_to_the_sums_over_the_fine_field(engine, scene, grid, k, level):
    want = fine_moments(scene, grid, k, level)
    axes = ref.grid_for(scene, grid)
    mp = run(scene, grid, k, level, density=2.0)
    assert mp.index_moments == want and all(type(v) is int for v in mp.index_moments)
    assert mp.dims == len(axes) and len(want) == (10 if mp.dims == 3 else 6)
    assert mp.shape == tuple(a.size for a in axes) and mp.samples == k and mp.inside_samples == want[0]
    assert 0 <= mp.near_cells <= int(np.prod(mp.shape))
    if scene == "cfg3":
        assert mp.near_cells == int(np.prod(mp.shape))
    # ... and the host conversion is the rational restatement (8 ulp at the quantity's scale: test_moments_cpu)
    world = mref.world(want, axes, k, 2.0)
    if want[0] == 0:                                            # (the eight corner samples of 2^3 with k = 1 can all be outside)
        assert mp.volume == 0.0 and np.all(np.isnan(mp.centroid)) and not mp.second_moments.any()
        return
    lo =np.array([a[0] - ((a[-1] - a[0]) / (a.size - 1)) / 2.0 for a in axes])
    assert mref.ulp_distance(mp.volume, world["volume"]) <= 8 and mref.ulp_distance(mp.mass, world["mass"]) <= 8
    assert mref.ulp_distance(mp.centroid, world["centroid"], scale=np.abs(lo)) <= 8
    scale = np.abs(np.diag(world["second_moments"])).max()
    assert mref.ulp_distance(mp.second_moments, world["second_moments"], scale=scale) <= 8


# ---- 2. modes, slabs and runs agree -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,grid,k,slab", [("cfg2", "17^3", 4, 2000), ("cfg2", "17^3", 8, 2000), ("sheared", "5x5x67", 4, 67),
                                               ("union300", "17^3", 2, 2000), ("cfg3", "3x5x7", 4, 7), ("cfg4", "65x63", 2, 63),
                                               ("cfg4", "3x130", 8, 130)])
def test_modes_slabs_and_runs_agree(engine, scene, grid, k, slab):
    level = 0.0
    want = fine_moments(scene, grid, k, level)
    got = {}
    with mode(_engine.MODE_SPECIALIZED):
        got["specialized"] = run(scene, grid, k, level)
    got["auto after the build"] = run(scene, grid, k, level)
    got["again"] = run(scene, grid, k, level)
    with mode(_engine.MODE_INTERPRET):
        got["interpret"] = run(scene, grid, k, level)
    with mode(_engine.MODE_NOCULL):
        got["nocull"] = run(scene, grid, k, level)
    n = int(np.prod([a.size for a in ref.grid_for(scene, grid)]))
    assert slab < n                                             # (17^3 in slabs of 117 rows; the others one row per slab)
    got["slabs"] = run(scene, grid, k, level, _slab_cells=slab)
    with mode(_engine.MODE_INTERPRET):
        got["slabs, interpreter"] = run(scene, grid, k, level, _slab_cells=slab)
    with mode(_engine.MODE_NOCULL):
        got["slabs, nocull"] = run(scene, grid, k, level, _slab_cells=slab)
    for name, mp in got.items():
        assert mp.index_moments == want, name
    assert got["nocull"].near_cells == got["slabs, nocull"].near_cells == n
    assert (got["slabs"].near_cells == got["specialized"].near_cells == got["interpret"].near_cells == got["again"].near_cells
            == got["slabs, interpreter"].near_cells)
    assert got["slabs"].volume == got["specialized"].volume == got["nocull"].volume
    assert np.array_equal(got["slabs"].inertia if got["slabs"].dims == 3 else got["slabs"].second_moments,
                          got["nocull"].inertia if got["nocull"].dims == 3 else got["nocull"].second_moments)


# ---- 3. the same classification as occupancy ----------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,grid,k,level", [("cfg1", "17^3", 4, 0.0), ("cfg2", "17^3", 4, 0.0), ("cfg5", "5x5x67", 2, 0.05),
                                                ("sheared", "33x31x64", 2, 0.0), ("union300", "17^3", 4, -0.03),
                                                ("cfg3", "3x5x7", 4, 0.0), ("cfg4", "65x63", 4, 0.0)])
def test_same_classification_as_occupancy(engine, scene, grid, k, level):
    occ = occupancy.fractions(ref.build(scene), ref.grid_for(scene, grid), k, level)
    mp = run(scene, grid, k, level)
    assert mp.inside_samples == occ.inside_samples and mp.near_cells == occ.near_cells
    if scene != "cfg3":
        assert 0 < mp.near_cells < occ.fraction.size
    # occupancy's volume: float64 row sums over the cells — 4 cells 2^-53 relative at the most
    assert abs(mp.volume - occ.volume) <= 4 * occ.fraction.size * 2.0 ** -53 * occ.volume


def test_a_larger_explicit_bound_gives_the_same_integers_and_more_near_cells(engine):
    L = lower_geometry(ref.build("cfg2")).lipschitz
    derived = run("cfg2", "17^3", 4, 0.0)
    same = run("cfg2", "17^3", 4, 0.0, lipschitz=L)
    twice = run("cfg2", "17^3", 4, 0.0, lipschitz=2.0 * L)
    assert twice.index_moments == derived.index_moments == same.index_moments == fine_moments("cfg2", "17^3", 4, 0.0)
    assert same.near_cells == derived.near_cells < twice.near_cells


# ---- 4. against the float64 oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["cfg1", "cfg2", "sheared"])
def test_moments_against_the_oracle(engine, scene):
    """Each integer moment differs from the oracle's by at most the sum of its term over the knife-edge sub-samples (those
    an fp32 evaluation may put on either side; the terms are positive)."""
    axes = ref.grid_for(scene, "17^3")
    inside, knife = mref.oracle_fields(ref.build(scene), axes, 4, 0.0)
    want, slack = mref.lattice_moments(inside, axes, 4), mref.lattice_moments(knife, axes, 4)
    assert slack[0] <= 8, "a badly chosen input: %d knife-edge sub-samples" % slack[0]
    got = run(scene, "17^3", 4, 0.0).index_moments
    print("%s: %d knife-edge sub-samples; moments - oracle's: %s" % (scene, slack[0], [g - w for g, w in zip(got, want)]))
    assert all(abs(g - w) <= s for g, w, s in zip(got, want, slack))


# ---- 5. closed forms ----------------------------------------------------------------------------------------------------------
def _box_inertia(mass, edge):
    return np.diag([mass * (edge[1] ** 2 + edge[2] ** 2) / 12.0, mass * (edge[0] ** 2 + edge[2] ** 2) / 12.0,
                    mass * (edge[0] ** 2 + edge[1] ** 2) / 12.0])


def test_an_aligned_box_has_its_closed_forms(engine):
    """The box of test_gpu_occupancy.test_volume_of_an_aligned_box_is_exact: faces on fine-cell boundaries (multiples of
    1 / 32 on a 17^3 grid over [-1, 1]^3 with k = 4). Step, origin and sub-cell are exact in float64, the integers are
    exact: 8 ulp — for the centroid, whose closed form is 0, of the lattice's origin it is added to."""
    axes = [np.linspace(-1, 1, 17)] * 3
    mp = moments.moments(ns.Box(0.5, 0.75, 0.25), axes, samples=4, density=3.0)
    edge = (0.5, 0.75, 0.25)
    assert mp.inside_samples == 16 * 24 * 8 and 0 < mp.near_cells < 17 ** 3
    assert mref.ulp_distance(mp.volume, 0.5 * 0.75 * 0.25) <= 8 and mref.ulp_distance(mp.mass, 3.0 * 0.5 * 0.75 * 0.25) <= 8
    assert mref.ulp_distance(mp.centroid, np.zeros(3), scale=1.0625) <= 8
    want = _box_inertia(3.0 * 0.5 * 0.75 * 0.25, edge)
    assert mref.ulp_distance(np.diag(mp.inertia), np.diag(want)) <= 8
    assert mref.ulp_distance(mp.inertia, want, scale=np.diag(want).max()) <= 8
    values, _ = mp.principal()
    assert mref.ulp_distance(values, np.sort(np.diag(want))) <= 8


def test_a_solid_that_fills_the_grid_is_the_grids_box(engine):
    """A sphere of radius 10 on 3 x 5 x 7 points over [-1.1, 1.1]^3: every cell is far and inside, nothing is sampled, and
    the solid is the box of the grid with its half-step overhang: n h per axis, centred where the grid is."""
    axes = ref.GRIDS["3x5x7"]
    mp = moments.moments(ns.Sphere(10.0), axes, samples=4, density=1.5)
    assert mp.near_cells == 0 and mp.inside_samples == 105 * 64
    assert mp.index_moments == mref.box_moments((0, 0, 0), (12, 20, 28))
    step = [(a[-1] - a[0]) / (a.size - 1) for a in axes]
    edge = [a.size * h for a, h in zip(axes, step)]
    volume = edge[0] * edge[1] * edge[2]
    assert mref.ulp_distance(mp.volume, volume) <= 8 and mref.ulp_distance(mp.mass, 1.5 * volume) <= 8
    lo = np.array([a[0] - h / 2.0 for a, h in zip(axes, step)])
    assert mref.ulp_distance(mp.centroid, lo + np.array(edge) / 2.0, scale=np.abs(lo)) <= 8
    want = _box_inertia(1.5 * volume, edge)
    assert mref.ulp_distance(np.diag(mp.inertia), np.diag(want)) <= 8 and np.all(mp.inertia[~np.eye(3, dtype=bool)] == 0.0)
    with mode(_engine.MODE_NOCULL):                             # every cell sampled: the same integers
        assert moments.moments(ns.Sphere(10.0), axes, samples=4).index_moments == mp.index_moments


def test_a_solid_outside_the_grid_is_empty(engine):
    sphere = ns.Sphere(0.5)
    sphere.move((5.0, 0.0, 0.0))
    mp = moments.moments(sphere, ref.GRIDS["3x5x7"], samples=2)
    assert mp.index_moments == (0,) * 10 and mp.near_cells == 0
    assert mp.volume == 0.0 and mp.mass == 0.0 and np.all(np.isnan(mp.centroid))
    assert not mp.inertia.any() and not mp.second_moments.any()
    circle = ns.Circle(0.5)
    circle.move((50.0, 0.0, 0.0))
    flat = moments.moments(circle, ref.GRIDS_2D["3x130"], samples=4)
    assert flat.index_moments == (0,) * 6 and flat.polar == 0.0 and flat.dims == 2


def test_a_sphere_lies_between_its_shells(engine):
    """radius r = 0.5 on 33^3 points over [-0.5, 0.5]^3, k = 4. The solid is the union of the sub-cells whose centre the
    fp32 field puts inside. A point within r - delta of the origin lies in a sub-cell whose centre is within half a
    sub-cell diagonal of it, so inside the exact sphere by more than eps, so inside for the fp32 field; a sub-cell whose
    centre the fp32 field puts inside lies within r + delta. delta = half the sub-cell diagonal + eps, eps = the absolute
    slack of the far rule, 1e-6 (1 + |f| + |level|) + 1e-6 (|cx| + |cy| + |cz|) <= 1e-6 (1 + 0.5 + 3 * 0.52): float32
    rounding of the sample's coordinates and of the field there. ball(r - delta) <= solid <= ball(r + delta) bounds the
    volume, and tr(I) = 2 int |x - c|^2 dm too: about its own centroid c a body's integral is the smallest about any
    point, so it is at most the integral about the origin, which grows with the set; and it is at least the inner ball's
    about c, which is at least the inner ball's about its own centre."""
    mp = moments.from_geometry(ns.Sphere(0.5), (1, 1, 1), (33, 33, 33), samples=4)
    s = (1.0 / 32.0) / 4.0
    delta = 0.5 * np.sqrt(3.0) * s + 1e-6 * (1.0 + 0.5 + 3 * 0.52)
    inner, outer = 0.5 - delta, 0.5 + delta
    trace = float(np.trace(mp.inertia))
    print("sphere: volume %.9f in [%.9f, %.9f]; tr(I) %.9f in [%.9f, %.9f]; centroid %s; %d near cells" %
          (mp.volume, 4 * np.pi / 3 * inner ** 3, 4 * np.pi / 3 * outer ** 3, trace, 8 * np.pi / 5 * inner ** 5,
           8 * np.pi / 5 * outer ** 5, mp.centroid, mp.near_cells))
    assert 4.0 * np.pi / 3.0 * inner ** 3 <= mp.volume <= 4.0 * np.pi / 3.0 * outer ** 3
    assert 8.0 * np.pi / 5.0 * inner ** 5 <= trace <= 8.0 * np.pi / 5.0 * outer ** 5
    # the inner ball adds nothing to int x dV, the rest lies within `outer` of the origin and the volume is at least the
    # inner ball's: |c| <= outer (V_outer - V_inner) / V_inner
    assert np.linalg.norm(mp.centroid) <= outer * (outer ** 3 - inner ** 3) / inner ** 3
    assert 0 < mp.near_cells < 33 ** 3 // 4


# ---- 6. the rest --------------------------------------------------------------------------------------------------------------
def test_from_geometry_is_moments_on_grid_axes(engine):
    geo = ref.build("cfg2")
    a = moments.from_geometry(geo, (2, 2, 2), (17, 19, 21), samples=2, level=0.05, density=4.0)
    axes, _ = ns.helper_functions.grid_axes((2, 2, 2), (17, 19, 21))
    b = moments.moments(geo, axes, samples=2, level=0.05, density=4.0)
    grid, _ = ns.generate_grid((2, 2, 2), (17, 19, 21))
    c = moments.moments(geo, grid, samples=2, level=0.05, density=4.0)
    for other in (b, c):
        assert (a.shape, a.index_moments, a.near_cells, a.volume, a.mass) == (other.shape, other.index_moments, other.near_cells,
                                                                              other.volume, other.mass)
        assert np.array_equal(a.inertia, other.inertia) and np.array_equal(a.centroid, other.centroid)
    assert a.density == 4.0 and a.mass == 4.0 * a.volume and a.level == float(np.float32(0.05))
    flat = moments.from_geometry(ref.build("cfg4"), (10, 10), (65, 63), samples=2)
    assert flat.index_moments == run("cfg4", "65x63", 2, 0.0).index_moments and flat.shape == (65, 63)


def test_timings(engine):
    t = {}
    run("cfg2", "17^3", 4, 0.0, timings=t)
    assert set(t) == {"centre", "far", "sample"} and all(v >= 0.0 for v in t.values())
