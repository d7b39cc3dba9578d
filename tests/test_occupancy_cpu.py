"""aegolius_amd.occupancy without a GPU: the sub-sample tables against tests/occupancy_reference.py bit for bit, every
refusal, the occupancy flavour's build, the new entry points, and the skip rule in float64 over the oracle."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import aegolius_amd.cores as ns
import occupancy_reference as ref
from aegolius_amd import occupancy, workloads
from aegolius_amd._lower import lower_geometry
from aegolius_amd.autodiff import UnsupportedOpError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _two_point():
    return [np.array([-0.3, 0.9]), np.linspace(-1, 1, 5), np.array([0.0, 1e-3])]


TABLE_GRIDS = {"uniform": ref.GRIDS["17^3"], "5x5x67": ref.GRIDS["5x5x67"], "nonuniform": ref.GRIDS["nonuniform"],
               "two-point": _two_point(), "2-D": ref.GRIDS_2D["65x63"], "moved": ref.grid_for("cfg2+1000", "17^3")}


@pytest.mark.parametrize("name", list(TABLE_GRIDS))
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_sample_tables_are_the_references(name, k):
    axes = TABLE_GRIDS[name]
    tabs, half = occupancy.sample_tables(axes, k)
    assert len(tabs) == len(half) == len(axes)
    for a, t, h in zip(axes, tabs, half):
        want = ref.table(a, k)
        assert t.dtype == np.float32 and h.dtype == np.float32 and t.shape == (a.size * k,) and h.shape == (a.size,)
        assert np.array_equal(t.view(np.uint32), want.view(np.uint32))
        hw = ref.half_width(a, k)
        assert np.all(h.astype(np.float64) >= hw)                          # never below the float64 value ...
        assert np.all(np.nextafter(h, np.float32(-np.inf)).astype(np.float64) < hw) or k == 1     # ... and the next float32 is
        assert np.all(np.diff(t.astype(np.float64)) > 0)


def test_sample_tables_of_a_2d_generate_grid():
    grid, _ = ns.generate_grid((10, 10), (65, 63))
    tabs, half = occupancy.sample_tables(grid, 2)
    assert [t.size for t in tabs] == [130, 126, 1] and tabs[2][0] == 0.0 and half[2][0] == 0.0
    for a, t in zip(ref.GRIDS_2D["65x63"], tabs):
        assert np.array_equal(t, ref.table(a, 2))
    two, _ = occupancy.sample_tables(ref.GRIDS_2D["65x63"], 2)
    assert len(two) == 2 and np.array_equal(two[0], tabs[0]) and np.array_equal(two[1], tabs[1])


def test_end_cells_overhang_by_half_a_step():
    lo, hi = ref.cells(np.linspace(-1, 1, 5))
    assert lo[0] == -1.25 and hi[-1] == 1.25 and np.array_equal(lo[1:], hi[:-1])
    tabs, _ = occupancy.sample_tables([np.linspace(-1, 1, 5)] * 3, 2)
    assert tabs[0][0] == np.float32(-1.125) and tabs[0][-1] == np.float32(1.125)


def test_refusals_need_no_gpu(built):
    ax = ref.GRIDS["3x5x7"]
    sphere = ns.Sphere(0.5)
    for bad in (0, 3, 16, 2.5, None, True):
        with pytest.raises(ValueError, match="samples"):
            occupancy.fractions(sphere, ax, samples=bad)
        with pytest.raises(ValueError, match="samples"):
            occupancy.sample_tables(ax, bad)
    with pytest.raises(ValueError, match="NaN"):
        occupancy.fractions(sphere, ax, level=float("nan"))
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="lipschitz"):
            occupancy.fractions(sphere, ax, lipschitz=bad)
    with pytest.raises(ValueError, match="strictly increasing"):
        occupancy.fractions(sphere, [ax[0], ax[1][::-1], ax[2]])
    with pytest.raises(ValueError, match="at least 2"):
        occupancy.fractions(sphere, [ax[0], ax[1], np.array([0.5])])
    with pytest.raises(ValueError, match="axis tables"):
        occupancy.fractions(sphere, ax[:1])
    with pytest.raises(ValueError, match="tagged"):
        occupancy.fractions(sphere, np.zeros((3, 8)))
    fine = 1000.0 + np.arange(5) * 1.3e-4                                   # distinct as float32, the 8 sub-samples are not
    with pytest.raises(ValueError, match="axis 0.*too fine"):
        occupancy.fractions(sphere, [fine, ax[1], ax[2]], samples=8)
    with pytest.raises(ValueError, match="2 or 3"):
        occupancy.from_geometry(sphere, (2,), (9,))

    signed = ns.Circle(0.5)
    signed.signed((32, 32, 1))
    with pytest.raises(UnsupportedOpError, match="staged"):
        occupancy.fractions(signed, ref.GRIDS_2D["3x130"])
    custom = ns.Sphere(0.5)
    custom.custom_post_process(lambda u, k: u * k, (2.0,))
    with pytest.raises(UnsupportedOpError, match="staged"):
        occupancy.from_geometry(custom, (2, 2, 2), (9, 9, 9))


def test_an_unbounded_field_is_not_refused():
    """cfg 3 has no finite bound: render refuses it, here nothing is skipped instead (the bound handed on is inf)."""
    low = lower_geometry(workloads.cfg3_chain(ns))
    assert low.lipschitz == np.inf and occupancy._lipschitz(low, None) == np.inf
    assert occupancy._lipschitz(low, 2.5) == 2.5
    assert occupancy._lipschitz(lower_geometry(ns.Sphere(0.5)), None) == 1.0


def test_native_argument_checks(built):
    """The C entry validates on the host and launches nothing."""
    prog = built.Program.from_lowered(lower_geometry(ns.Sphere(0.5)))
    L = built.lib()
    ax = [np.linspace(-1, 1, 5, dtype=np.float32)] * 3
    tabs, half = occupancy.sample_tables(ax, 2)
    one = ctypes.c_void_p(4096)                                  # (never dereferenced: the calls fail first)
    inside, near = ctypes.c_int64(0), ctypes.c_int64(0)

    def call(samples=2, level=0.0, lip=1.0, out=one, mode=built.MODE_INTERPRET, handle=prog.handle):
        tab = []
        for a in ax:
            tab += [built._ptr(a), a.size]
        return L.sdfk_eval_grid_occupancy(handle, *tab, *[built._ptr(t) for t in tabs], *[built._ptr(h) for h in half], samples,
                                          level, lip, out, one, 0, ctypes.byref(inside), ctypes.byref(near), None, None, mode)
    assert call(samples=3) == -1 and "samples" in built.last_error()
    assert call(level=float("nan")) == -1 and "NaN" in built.last_error()
    assert call(lip=-1.0) == -1 and "Lipschitz" in built.last_error()
    assert call(lip=float("nan")) == -1
    assert call(out=None) == -1
    assert call(mode=7) == -1
    assert call(handle=None) == -1
    assert L.sdfk_field_row_sums(one, -1, 4, None, one, None) == -1
    # scratch: 8 bytes per slab cell (centre values, list), 8 per 1024 slab cells (counts) and 32 KB; slabs are whole rows
    def scratch(cells):
        return 32768 + ((-(-cells // 1024) + 1) * 8 + 255) // 256 * 256 + 2 * ((cells * 4 + 255) // 256 * 256)
    assert L.sdfk_eval_grid_occupancy_scratch(17, 17, 17, 0) == scratch(17 ** 3)
    assert L.sdfk_eval_grid_occupancy_scratch(17, 17, 17, 2000) == scratch(117 * 17)
    assert L.sdfk_eval_grid_occupancy_scratch(1025, 1025, 1025, 0) <= 8.01 * 1025 ** 3 + 33792
    assert L.sdfk_eval_grid_occupancy_scratch(2049, 2049, 2049, 0) <= 8.01 * 2 ** 30 + 33792


def test_new_entries_are_declared_and_exported(built):
    header = open(os.path.join(ROOT, "include", "sdfk.h")).read()
    for name in ("sdfk_eval_grid_occupancy_scratch", "sdfk_eval_grid_occupancy", "sdfk_field_row_sums"):
        assert name in built.SIGNATURES and hasattr(built.lib(), name) and name + "(" in header
    assert "#define SDFK_FLAVOUR_OCCUPANCY 11" in header and built.FLAVOUR_OCCUPANCY == 11
    assert built.lib().sdfk_abi_version() == 1
    assert callable(built.Program.occupancy_grid)
    import __graft_entry__
    assert "sdfk_occupancy.inc" in __graft_entry__.DEPS and "sdfk_occdev.h" in __graft_entry__.DEPS
    embedded = open(os.path.join(ROOT, "aegolius_amd", "csrc", "sdfk_embedded.inc")).read()
    assert "kEmbeddedOccdev" in embedded and "sdfk_occ_sample" in embedded


def test_occupancy_flavour_builds_for_gfx950(built):
    for tree, members in ((workloads.cfg2_tree(ns), 0), (workloads.sphere_union(ns, count=300), 300)):
        prog = built.Program.from_lowered(lower_geometry(tree))
        assert prog.chain_members == members                     # the union: the table-driven body
        size, _ = prog.compile_flavour(built.FLAVOUR_OCCUPANCY)
        assert size > 5000
        builds = built.jit_stats()[0]
        again, _ = prog.compile_flavour(built.FLAVOUR_OCCUPANCY)
        assert again == size and built.jit_stats()[0] == builds  # served from the cache: no hiprtc build ran
        with pytest.raises(built.SdfkError):
            prog.compile_flavour(built.FLAVOUR_OCCUPANCY | built.FLAVOUR_FLAGS)
    assert prog.compile_check() > 0                              # (the evaluation flavours: this one is not among them)


_NAMES_SCRIPT = """
import sys
sys.path.insert(0, %r)
import aegolius_amd.cores as ns
from aegolius_amd import _engine, workloads
from aegolius_amd._lower import lower_geometry
for tree in (workloads.cfg2_tree(ns), workloads.sphere_union(ns, count=300)):
    _engine.Program.from_lowered(lower_geometry(tree)).compile_flavour(_engine.FLAVOUR_OCCUPANCY)
"""


def test_occupancy_flavour_exports_its_kernels(built, tmp_path):
    """The code objects of the flavour, built by a fresh process into an on-disk cache of its own, carry the two kernels
    the launcher asks for by name (and none of the ray kernels)."""
    env = dict(os.environ, SDFK_CACHE_DIR=str(tmp_path))
    subprocess.run([sys.executable, "-c", _NAMES_SCRIPT % ROOT], check=True, env=env, timeout=600)
    blobs = [open(os.path.join(str(tmp_path), f), "rb").read() for f in sorted(os.listdir(str(tmp_path))) if f.endswith(".co")]
    assert len(blobs) == 2
    for blob in blobs:
        assert b"sdfk_spec_occ_list" in blob and b"sdfk_spec_occ_all" in blob and b"sdfk_spec_rays" not in blob


RULE_CASES = [(s, g, k, lv) for s in ref.BOUNDED for g in ("17^3", "5x5x67", "nonuniform") for k, lv in ((4, 0.0), (2, 0.05))]


@pytest.mark.parametrize("scene,grid,k,level", RULE_CASES)
def test_skip_rule_in_float64_over_the_oracle(scene, grid, k, level):
    """No partially covered cell outside the band |f(c) - level| <= L rho, and outside it the centre's side is the
    cell's: in exact arithmetic the rule follows from the Lipschitz bound; here it is checked on the oracle."""
    geo = ref.build(scene)
    axes = ref.grid_for(scene, grid)
    L = lower_geometry(geo).lipschitz
    assert np.isfinite(L)
    counts, _ = ref.oracle_counts(geo, axes, k, level)
    K = k ** 3
    dist, band = ref.centre_band(geo, axes, k, level, L)
    far = dist > band
    partial = (counts > 0) & (counts < K)
    assert not np.any(partial & far)
    ax32 = [a.astype(np.float32) for a in axes]
    from oracle import sdf_oracle
    centre_in = sdf_oracle.evaluate(geo, ref.grid_points(ax32)) <= float(np.float32(level))
    assert np.array_equal(counts[far], np.where(centre_in[far], K, 0))
    assert 0 < far.sum() < far.size or scene == "union300"
