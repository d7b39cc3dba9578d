"""aegolius_amd.occupancy on the GPU (kernels: csrc/sdfk_occupancy.inc, csrc/sdfk_occdev.h): equal, bit for bit, to the block
sum of the package's own field on the fine grid; the same under every mode, slab size and run; skipping happens; the float64
oracle; closed forms; the rest of the interface. Definition, scenes and grids: tests/occupancy_reference.py.

The shapes are the smallest that reach: a list length that is no multiple of the entries per wave, entries of one wave in
different rows and planes, eight rounds per cell (K = 512), 16 entries per wave (2-D, k = 2), and a slab seam."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import aegolius_amd.cores as ns  # noqa: E402
import occupancy_reference as ref  # noqa: E402
from aegolius_amd import _engine, occupancy  # noqa: E402
from aegolius_amd._eval import config, program_for  # noqa: E402
from aegolius_amd._lower import lower_geometry  # noqa: E402

pytestmark = pytest.mark.gpu

COMBOS = [("2^3", 1, 0.0), ("2^3", 4, 0.05), ("3x5x7", 2, 0.05), ("3x5x7", 4, 0.0), ("17^3", 1, 0.0), ("17^3", 2, -0.03),
          ("17^3", 4, 0.0), ("5x5x67", 4, -0.03), ("5x5x67", 2, 0.0), ("33x31x64", 2, 0.05), ("33x31x64", 1, 0.0),
          ("nonuniform", 4, 0.05), ("nonuniform", 2, 0.0), ("9^3", 8, 0.0)]
COMBOS_2D = [("65x63", 1, -0.03), ("65x63", 2, 0.0), ("65x63", 4, 0.05), ("3x130", 2, 0.05), ("3x130", 4, 0.0), ("3x130", 8, 0.0)]
CASES = [(s, g, k, lv) for s in ref.SCENES for g, k, lv in COMBOS] + [(s, g, k, lv) for s in ref.SCENES_2D for g, k, lv in COMBOS_2D]


class mode:
    def __init__(self, m):
        self.m = m

    def __enter__(self):
        self.old, config.mode = config.mode, self.m

    def __exit__(self, *exc):
        config.mode = self.old


@functools.lru_cache(maxsize=None)
def fine_counts(scene, grid, k, level):
    """Counts per cell from the package's existing path: Program.eval_grid of the fine grid the reference's tables span,
    downloaded, compared with the level and block-summed on the host."""
    axes = ref.grid_for(scene, grid)
    tabs = ref.tables(axes, k)
    n = int(np.prod([t.size for t in tabs]))
    prog = program_for(lower_geometry(ref.build(scene)))
    with _engine.DeviceField(n, config.device) as field:
        prog.eval_grid(tabs, 0, n, field.ptr, mode=config.mode)
        _engine.check(_engine.lib().sdfk_sync(None), "sdfk_sync")
        values = field.numpy()
    with np.errstate(invalid="ignore"):
        counts = ref.block_sum(values <= np.float32(level), axes, k)
    counts.setflags(write=False)
    return counts


def K_of(scene, k):
    return k ** (2 if scene in ref.SCENES_2D else 3)


def run(scene, grid, k, level, **kw):
    return occupancy.fractions(ref.build(scene), ref.grid_for(scene, grid), k, level, **kw)


# ---- 1. equal to the existing path, bit for bit -------------------------------------------------------------------------
@pytest.mark.parametrize("scene,grid,k,level", CASES)
def test_equal_to_the_block_sum_of_the_fine_field(engine, scene, grid, k, level):
    counts = fine_counts(scene, grid, k, level)
    K = K_of(scene, k)
    occ = run(scene, grid, k, level)
    assert occ.fraction.dtype == np.float32 and occ.fraction.shape == counts.shape
    assert occ.shape == tuple(a.size for a in ref.grid_for(scene, grid)) and occ.samples == k
    np.testing.assert_array_equal(occ.fraction, (counts / K).astype(np.float32))
    assert occ.inside_samples == int(counts.sum()) and isinstance(occ.inside_samples, int)
    assert 0 <= occ.near_cells <= counts.size


# ---- 2. skipping changes nothing ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,grid,k", [("cfg2", "17^3", 4), ("cfg2", "17^3", 2), ("sheared", "5x5x67", 4), ("union300", "17^3", 4),
                                          ("cloud300", "nonuniform", 2), ("cfg3", "3x5x7", 4), ("cfg4", "65x63", 2),
                                          ("cfg2", "9^3", 8)])
def test_modes_slabs_and_runs_agree(engine, scene, grid, k):
    level = 0.0
    counts = fine_counts(scene, grid, k, level)
    want = (counts / K_of(scene, k)).astype(np.float32)
    got = {}
    with mode(_engine.MODE_SPECIALIZED):
        got["specialized"] = run(scene, grid, k, level)
    got["auto after the build"] = run(scene, grid, k, level)
    got["again"] = run(scene, grid, k, level)
    with mode(_engine.MODE_INTERPRET):
        got["interpret"] = run(scene, grid, k, level)
    with mode(_engine.MODE_NOCULL):
        got["nocull"] = run(scene, grid, k, level)
    n = counts.size
    row = ref.grid_for(scene, grid)[-1].size                    # slabs are whole rows: a third of the rows, rounded up
    slab = -(-(n // row) // 3) * row
    assert slab < n and -(-n // slab) == 3                       # (17^3: 1649 + 1649 + 1615 cells, two seams)
    got["three slabs"] = run(scene, grid, k, level, _slab_cells=slab)
    with mode(_engine.MODE_INTERPRET):
        got["three slabs, interpreter"] = run(scene, grid, k, level, _slab_cells=slab)
    for name, occ in got.items():
        np.testing.assert_array_equal(occ.fraction, want, err_msg=name)
        assert occ.inside_samples == int(counts.sum()), name
    assert got["nocull"].near_cells == n
    assert got["three slabs"].near_cells == got["specialized"].near_cells == got["interpret"].near_cells == got["again"].near_cells
    assert got["three slabs"].volume == got["specialized"].volume == got["nocull"].volume


# ---- 3. skipping happens --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["cfg1", "cfg2", "sheared"])
@pytest.mark.parametrize("grid,k", [("17^3", 4), ("33x31x64", 2)])
def test_near_cells_between_the_partial_cells_and_the_band(engine, scene, grid, k):
    geo = ref.build(scene)
    axes = ref.grid_for(scene, grid)
    counts = fine_counts(scene, grid, k, 0.0)
    K = k ** 3
    partial = int(np.count_nonzero((counts > 0) & (counts < K)))
    dist, band = ref.centre_band(geo, axes, k, 0.0, lower_geometry(geo).lipschitz)
    bound = int(np.count_nonzero(dist <= 1.01 * band + 1e-5))
    occ = run(scene, grid, k, 0.0)
    print("%s %s k=%d: %d partially covered cells <= %d near cells <= %d in the oracle's band (%.1f %% of %d cells)" %
          (scene, grid, k, partial, occ.near_cells, bound, 100.0 * bound / counts.size, counts.size))
    assert partial <= occ.near_cells <= bound < counts.size


def test_nothing_is_skipped_without_a_bound(engine):
    occ = run("cfg3", "17^3", 2, 0.0)
    assert occ.near_cells == 17 ** 3
    with mode(_engine.MODE_NOCULL):
        assert run("cfg2", "17^3", 2, 0.0).near_cells == 17 ** 3
    assert run("cfg2", "17^3", 2, 0.0).near_cells < 17 ** 3 // 2


# ---- 4. against the float64 oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,grid,k,level", [("cfg1", "17^3", 4, 0.0), ("cfg2", "17^3", 4, 0.0), ("cfg5", "17^3", 4, 0.0),
                                                ("sheared", "17^3", 4, 0.0), ("union300", "9^3", 4, 0.0),
                                                ("cfg2", "nonuniform", 2, 0.05), ("cfg5", "5x5x67", 4, -0.03),
                                                ("sheared", "33x31x64", 2, 0.0), ("cfg4", "65x63", 2, 0.0),
                                                ("cfg4", "3x130", 4, 0.05)])
def test_counts_against_the_oracle(engine, scene, grid, k, level):
    """|count - oracle count| <= the knife-edge sub-samples of the cell (those an fp32 evaluation may put on either side)."""
    want, knife = ref.oracle_counts(ref.build(scene), ref.grid_for(scene, grid), k, level)
    assert knife.sum() <= 8, "a badly chosen input: %d knife-edge sub-samples" % knife.sum()
    occ = run(scene, grid, k, level)
    got = np.rint(occ.fraction.astype(np.float64) * K_of(scene, k)).astype(np.int64)
    print("%s %s k=%d level %g: %d knife-edge sub-samples, %d cells differ from the oracle" %
          (scene, grid, k, level, knife.sum(), np.count_nonzero(got != want)))
    assert np.all(np.abs(got - want) <= knife)


# ---- 5. closed forms ------------------------------------------------------------------------------------------------------
def test_volume_of_a_sphere(engine):
    """radius 0.5 on 33^3 points over [-0.5, 0.5]^3, k = 4: one fine step is 1 / 64 of the radius; the staircase error of
    a sphere's volume is of the order of (fine step / radius) / sqrt(number of steps) — far inside the 1 % asked for."""
    occ = occupancy.from_geometry(ns.Sphere(0.5), (1, 1, 1), (33, 33, 33), samples=4)
    exact = 4.0 * np.pi / 3.0 * 0.125
    print("sphere: volume %.9f, exact %.9f, relative error %.3e; %d near cells of %d" %
          (occ.volume, exact, abs(occ.volume - exact) / exact, occ.near_cells, 33 ** 3))
    assert abs(occ.volume - exact) <= 0.01 * exact
    assert occ.inside_samples == int(round(float(occ.fraction.astype(np.float64).sum() * 64)))


def test_volume_of_an_aligned_box_is_exact(engine):
    """Faces on fine-cell boundaries (multiples of 1 / 32 on a 17^3 grid over [-1, 1]^3 with k = 4), every sample at least
    half a fine step from a face: the volume is the box's, to rounding."""
    axes = [np.linspace(-1, 1, 17)] * 3
    occ = occupancy.fractions(ns.Box(0.5, 0.75, 0.25), axes, samples=4)
    assert abs(occ.volume - 0.5 * 0.75 * 0.25) <= 1e-12 * 0.5 * 0.75 * 0.25
    assert occ.inside_samples == 16 * 24 * 8
    assert set(np.unique(occ.fraction)) <= {0.0, 0.5, 1.0, 0.25, 0.125}


@pytest.mark.parametrize("scene,grid,k", [("cfg2", "nonuniform", 4), ("cfg5", "17^3", 2), ("cfg4", "65x63", 4)])
def test_volume_is_the_float64_sum_of_its_terms(engine, scene, grid, k):
    occ = run(scene, grid, k, 0.0)
    want = float(np.sum(occ.fraction.astype(np.float64) * ref.cell_volumes(ref.grid_for(scene, grid))))
    assert want > 0.0 and abs(occ.volume - want) <= 1e-12 * want          # (n 2^-53 with n <= 8000 cells)


# ---- 6. the rest ----------------------------------------------------------------------------------------------------------
def test_resident_result(engine):
    host = run("cfg2", "17^3", 4, 0.0)
    dev = run("cfg2", "17^3", 4, 0.0, resident=True)
    assert isinstance(dev.fraction, _engine.DeviceField) and dev.fraction.n == 17 ** 3
    np.testing.assert_array_equal(dev.fraction.numpy(), host.fraction)
    assert (dev.inside_samples, dev.near_cells, dev.volume) == (host.inside_samples, host.near_cells, host.volume)
    dev.free()
    assert dev.fraction.ptr is None


def test_from_geometry_is_fractions_on_grid_axes(engine):
    geo = ref.build("cfg2")
    a = occupancy.from_geometry(geo, (2, 2, 2), (17, 19, 21), samples=2, level=0.05)
    axes, _ = ns.helper_functions.grid_axes((2, 2, 2), (17, 19, 21))
    b = occupancy.fractions(geo, axes, samples=2, level=0.05)
    grid, _ = ns.generate_grid((2, 2, 2), (17, 19, 21))
    c = occupancy.fractions(geo, grid, samples=2, level=0.05)
    for other in (b, c):
        np.testing.assert_array_equal(a.fraction, other.fraction)
        assert (a.shape, a.inside_samples, a.near_cells, a.volume) == (other.shape, other.inside_samples, other.near_cells, other.volume)
    flat = occupancy.from_geometry(ref.build("cfg4"), (10, 10), (65, 63), samples=2)
    np.testing.assert_array_equal(flat.fraction, run("cfg4", "65x63", 2, 0.0).fraction)
    assert flat.shape == (65, 63)


def test_a_larger_explicit_bound_gives_the_same_bits_and_more_near_cells(engine):
    geo = ref.build("cfg2")
    L = lower_geometry(geo).lipschitz
    derived = run("cfg2", "17^3", 4, 0.0)
    same = run("cfg2", "17^3", 4, 0.0, lipschitz=L)
    twice = run("cfg2", "17^3", 4, 0.0, lipschitz=2.0 * L)
    np.testing.assert_array_equal(twice.fraction, derived.fraction)
    assert twice.inside_samples == derived.inside_samples and same.near_cells == derived.near_cells
    assert twice.near_cells > derived.near_cells


def test_timings(engine):
    t = {}
    run("cfg2", "17^3", 4, 0.0, timings=t)
    assert set(t) == {"centre", "classify", "sample", "volume"} and all(v >= 0.0 for v in t.values())
