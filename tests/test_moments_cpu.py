"""aegolius_amd.moments without a GPU: every refusal, the host conversion of integer moments against closed forms and against
the rational restatement of tests/moments_reference.py, the parallel-axis theorem and the principal axes, the C entry's
argument checks, the declarations, and the moments flavour's build."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import aegolius_amd.cores as ns
import moments_reference as mref
import occupancy_reference as ref
from aegolius_amd import moments, occupancy, workloads
from aegolius_amd._lower import lower_geometry
from aegolius_amd.autodiff import UnsupportedOpError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_need_no_gpu(built):
    ax = ref.GRIDS["3x5x7"]
    sphere = ns.Sphere(0.5)
    with pytest.raises(ValueError, match="uniform"):
        moments.moments(sphere, ref.GRIDS["nonuniform"])
    bent = [ax[0], ax[1], ax[2] + 1e-5 * ax[2] ** 2]             # 1e-5 of the extent off a line: 3e-5 of a step
    with pytest.raises(ValueError, match="axis 2 is not uniform.*occupancy.fractions"):
        moments.moments(sphere, bent)
    for bad in (0, 3, 16, 2.5, None, True):
        with pytest.raises(ValueError, match="samples"):
            moments.moments(sphere, ax, samples=bad)
    with pytest.raises(ValueError, match="NaN"):
        moments.moments(sphere, ax, level=float("nan"))
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="lipschitz"):
            moments.moments(sphere, ax, lipschitz=bad)
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="density"):
            moments.moments(sphere, ax, density=bad)
    with pytest.raises(ValueError, match="strictly increasing"):
        moments.moments(sphere, [ax[0], ax[1][::-1], ax[2]])
    with pytest.raises(ValueError, match="at least 2"):
        moments.moments(sphere, [ax[0], ax[1], np.array([0.5])])
    with pytest.raises(ValueError, match="axis tables"):
        moments.moments(sphere, ax[:1])
    with pytest.raises(ValueError, match="tagged"):
        moments.moments(sphere, np.zeros((3, 8)))
    fine = 1000.0 + np.arange(5) * 1.3e-4                                   # distinct as float32, the 8 sub-samples are not
    with pytest.raises(ValueError, match="axis 0.*too fine"):
        moments.moments(sphere, [fine, ax[1], ax[2]], samples=8)
    with pytest.raises(ValueError, match="2 or 3"):
        moments.from_geometry(sphere, (2,), (9,))

    signed = ns.Circle(0.5)
    signed.signed((32, 32, 1))
    with pytest.raises(UnsupportedOpError, match="staged"):
        moments.moments(signed, ref.GRIDS_2D["3x130"])
    custom = ns.Sphere(0.5)
    custom.custom_post_process(lambda u, k: u * k, (2.0,))
    with pytest.raises(UnsupportedOpError, match="staged"):
        moments.from_geometry(custom, (2, 2, 2), (9, 9, 9))


def test_the_module_is_not_imported_by_the_package():
    code = "import sys; import aegolius_amd; assert 'aegolius_amd.moments' not in sys.modules"
    subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); %s" % (ROOT, code)], check=True, timeout=300)


# ---- the reference itself -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axes,k", [(ref.GRIDS["2^3"], 2), (ref.GRIDS["3x5x7"], 1), (ref.GRIDS["3x5x7"], 2),
                                    (ref.GRIDS_2D["3x130"], 2)])
def test_lattice_moments_are_the_sums_over_the_samples(axes, k):
    fine = [a.size * kk for a, kk in zip(ref.three(axes), ref.per_axis(axes, k))]
    inside = np.random.default_rng(3).uniform(size=fine) < 0.3
    got = mref.lattice_moments(inside, axes, k)
    assert got == mref.brute_moments(inside, axes, k) and all(type(v) is int for v in got)
    assert len(got) == (10 if len(axes) == 3 else 6)
    whole = mref.lattice_moments(np.ones(fine, dtype=bool), axes, k)
    assert whole == mref.box_moments([0] * len(axes), fine[:len(axes)])


# ---- host conversion --------------------------------------------------------------------------------------------------------
STEP = (0.3, 0.125, 0.07)                  # the grid steps h; with k = 2 the sub-cells are half of them
BOX = (4, 6, 10)                           # sub-cells per axis


def _box(first, density=2.5, k=2):
    """MassProperties of the box of BOX sub-cells whose lowest sub-cell has the fine indices `first`, on a lattice with
    lo = 0, from synthetic integer moments; and its closed forms in float64."""
    M = mref.box_moments(first, BOX)
    mp = moments.MassProperties(M, (0.0, 0.0, 0.0), STEP, (8, 8, 8), k, 0.0, density, 0)
    s = [h / k for h in STEP]
    edge = [c * x for c, x in zip(BOX, s)]
    volume = edge[0] * edge[1] * edge[2]
    mass = density * volume
    centre = np.array([(f + c / 2.0) * x for f, c, x in zip(first, BOX, s)])
    inertia = np.diag([mass * (edge[1] ** 2 + edge[2] ** 2) / 12.0, mass * (edge[0] ** 2 + edge[2] ** 2) / 12.0,
                       mass * (edge[0] ** 2 + edge[1] ** 2) / 12.0])
    return mp, volume, mass, centre, inertia


def test_a_box_a_million_steps_from_the_origin_has_its_closed_forms():
    """Exact integers, then a few roundings: 8 ulp. N U_ab - U_a U_b is about 1e-12 of either product here; formed in
    float64 it would be noise."""
    far, volume, mass, centre, inertia = _box((10 ** 6, 2 * 10 ** 6, 3 * 10 ** 6))
    near, _, _, centre0, _ = _box((0, 0, 0))
    for mp, c in ((far, centre), (near, centre0)):
        assert mp.inside_samples == 240 and mp.dims == 3 and mp.index_moments[0] == 240
        assert mref.ulp_distance(mp.volume, volume) <= 8 and mref.ulp_distance(mp.mass, mass) <= 8
        assert mref.ulp_distance(mp.centroid, c) <= 8
        assert mref.ulp_distance(np.diag(mp.inertia), np.diag(inertia)) <= 8
        assert np.all(mp.inertia[~np.eye(3, dtype=bool)] == 0.0)
        assert np.array_equal(mp.second_moments, mp.second_moments.T)
    assert np.array_equal(far.inertia, near.inertia) and np.array_equal(far.second_moments, near.second_moments)
    U = far.index_moments
    assert abs(U[0] * U[4] - U[1] * U[1]) < 1e-11 * U[1] * U[1]          # (the cancellation that exact integers survive)


@pytest.mark.parametrize("dims", [2, 3])
def test_conversion_is_the_rational_restatement(dims):
    """A random solid: every quantity within 8 ulp of tests/moments_reference.world (exact rationals, rounded once), at the
    scale of the quantity — a centroid coordinate at the scale of the lattice's origin it is added to."""
    axes = [np.linspace(999.0, 1001.2, 12), np.linspace(-1.1, 1.1, 9), np.linspace(0.3, 0.9, 7)][:dims]
    k = 4
    fine = [a.size * kk for a, kk in zip(ref.three(axes), ref.per_axis(axes, k))]
    inside = np.random.default_rng(11).uniform(size=fine) < 0.2
    M = mref.lattice_moments(inside, axes, k)
    lo = [a[0] - ((a[-1] - a[0]) / (a.size - 1)) / 2.0 for a in axes]
    step = [(a[-1] - a[0]) / (a.size - 1) for a in axes]
    mp = moments.MassProperties(M, lo, step, [a.size for a in axes], k, 0.0, 7.5, 0)
    want = mref.world(M, axes, k, 7.5)
    assert mref.ulp_distance(mp.volume, want["volume"]) <= 8 and mref.ulp_distance(mp.mass, want["mass"]) <= 8
    assert mref.ulp_distance(mp.centroid, want["centroid"], scale=np.abs(lo)) <= 8
    scale = np.abs(np.diag(want["second_moments"])).max()
    assert mref.ulp_distance(mp.second_moments, want["second_moments"], scale=scale) <= 8
    if dims == 3:
        assert mref.ulp_distance(mp.inertia, want["inertia"], scale=scale) <= 8
    else:
        assert mref.ulp_distance(mp.polar, want["polar"]) <= 8 and not hasattr(mp, "inertia")


def test_parallel_axes_principal_moments_and_gyration():
    mp, volume, mass, centre, inertia = _box((3, 1, 2))
    point = np.array([0.7, -0.2, 1.5])
    r = point - mp.centroid
    want = mp.inertia + mp.mass * (float(r @ r) * np.eye(3) - np.outer(r, r))
    np.testing.assert_array_equal(mp.inertia_about(point), want)
    np.testing.assert_array_equal(mp.inertia_about(mp.centroid), mp.inertia)
    # about a corner of the box, closed form: I_xx = m (b^2 + c^2) / 3
    s = [h / 2 for h in STEP]
    corner = np.array([3 * s[0], 1 * s[1], 2 * s[2]])
    edge = [c * x for c, x in zip(BOX, s)]
    about = mp.inertia_about(corner)
    assert mref.ulp_distance(about[0, 0], mass * (edge[1] ** 2 + edge[2] ** 2) / 3.0) <= 16
    assert mref.ulp_distance(about[0, 1], -mass * edge[0] * edge[1] / 4.0) <= 16
    with pytest.raises(ValueError):
        mp.inertia_about((0.0, 0.0))
    values, vectors = mp.principal()
    assert np.all(np.diff(values) >= 0) and mref.ulp_distance(values, np.sort(np.diag(inertia))) <= 8
    assert np.allclose(np.abs(vectors), np.eye(3)[:, np.argsort(np.diag(inertia))])
    assert mref.ulp_distance(mp.radius_of_gyration, np.sqrt(np.diag(inertia) / mass)) <= 8
    # 2-D: a 4 x 6 rectangle of sub-cells
    flat = moments.MassProperties(mref.box_moments((5, 7), (4, 6)), (0.0, 0.0), STEP[:2], (8, 8), 2, 0.0, 1.0, 0)
    a, b = 4 * STEP[0] / 2, 6 * STEP[1] / 2
    assert flat.dims == 2 and mref.ulp_distance(flat.volume, a * b) <= 8
    assert mref.ulp_distance(flat.polar, a * b * (a * a + b * b) / 12.0) <= 8
    assert mref.ulp_distance(flat.inertia_about(flat.centroid + np.array([3.0, 4.0])), flat.polar + flat.mass * 25.0) <= 8
    values, _ = flat.principal()
    assert mref.ulp_distance(values, np.sort([a * b * a * a / 12.0, a * b * b * b / 12.0])) <= 8
    assert mref.ulp_distance(flat.radius_of_gyration, np.sqrt((a * a + b * b) / 12.0)) <= 8


@pytest.mark.parametrize("dims", [2, 3])
def test_the_empty_solid(dims):
    mp = moments.MassProperties((0,) * (10 if dims == 3 else 6), (0.0,) * dims, STEP[:dims], (8,) * dims, 4, 0.0, 3.0, 5)
    assert mp.volume == 0.0 and mp.mass == 0.0 and mp.inside_samples == 0 and mp.near_cells == 5
    assert mp.centroid.shape == (dims,) and np.all(np.isnan(mp.centroid))
    assert mp.second_moments.shape == (dims, dims) and not mp.second_moments.any()
    if dims == 3:
        assert mp.inertia.shape == (3, 3) and not mp.inertia.any() and not mp.inertia_about((1.0, 2.0, 3.0)).any()
        assert np.all(np.isnan(mp.radius_of_gyration))
    else:
        assert mp.polar == 0.0 and mp.inertia_about((1.0, 2.0)) == 0.0 and np.isnan(mp.radius_of_gyration)
    values, _ = mp.principal()
    assert not values.any()
    with pytest.raises(ValueError, match="integer moments"):
        moments.MassProperties((0,) * 7, (0.0,) * dims, STEP[:dims], (8,) * dims, 4, 0.0, 3.0, 0)


# ---- the native entry -------------------------------------------------------------------------------------------------------
def test_native_argument_checks(built):
    """The C entry validates on the host and launches nothing."""
    prog = built.Program.from_lowered(lower_geometry(ns.Sphere(0.5)))
    L = built.lib()
    ax = [np.linspace(-1, 1, 5, dtype=np.float32)] * 3
    tabs, half = occupancy.sample_tables(ax, 2)
    one = ctypes.c_void_p(4096)                                  # (never dereferenced: the calls fail first)
    words, near = (ctypes.c_uint64 * 20)(), ctypes.c_int64(0)
    need = L.sdfk_eval_grid_moments_scratch(5, 5, 5, 0)

    def call(samples=2, level=0.0, lip=1.0, scratch=one, nbytes=need, out=words, near_out=ctypes.byref(near),
             mode=built.MODE_INTERPRET, handle=prog.handle, tables=tabs):
        tab = []
        for a in ax:
            tab += [built._ptr(a), a.size]
        sub = [built._ptr(t) if t is not None else None for t in tables]
        return L.sdfk_eval_grid_moments(handle, *tab, *sub, *[built._ptr(h) for h in half], samples, level, lip, scratch,
                                        nbytes, 0, out, near_out, None, None, mode)
    assert call(samples=3) == -1 and "samples" in built.last_error()
    assert call(level=float("nan")) == -1 and "NaN" in built.last_error()
    assert call(lip=-1.0) == -1 and "Lipschitz" in built.last_error()
    assert call(lip=float("nan")) == -1
    assert call(scratch=None) == -1
    assert call(nbytes=need - 1) == -1 and "scratch" in built.last_error()
    assert call(out=None) == -1
    assert call(near_out=None) == -1
    assert call(tables=[tabs[0], None, tabs[2]]) == -1 and "table" in built.last_error()
    assert call(mode=7) == -1
    assert call(handle=None) == -1
    # an axis too long for 32-bit lattice coordinates, and one on which a 64-bit partial could wrap: 512 (2^31)^2 >= 2^63
    # (the tables are never read: the calls fail first)
    def long_axis(n0):
        return L.sdfk_eval_grid_moments(prog.handle, one, n0, one, 2, one, 2, one, one, one, one, one, one, 8, 0.0, 1.0, one,
                                        2 ** 62, 0, words, ctypes.byref(near), None, None, built.MODE_INTERPRET)
    assert long_axis(2 ** 28) == -1 and "2^31 sub-samples" in built.last_error()
    assert long_axis(2 ** 27) == -2 and "wrap" in built.last_error()
    assert not any(words) and near.value == 0
    # scratch: occupancy's 8 bytes per slab cell and 8 per 1024 slab cells, and two arrays of 80-byte partials — one per
    # wave, whole blocks of four waves, at most 65536: for the slab's cells and for its runs of 1024 cells
    def partials(units):
        return (-(-min(units, 65536) // 4) * 4 * 80 + 255) // 256 * 256

    def scratch(cells):
        runs = -(-cells // 1024)
        return partials(cells) + partials(runs) + ((runs + 1) * 8 + 255) // 256 * 256 + 2 * ((cells * 4 + 255) // 256 * 256)
    assert need == scratch(125)
    assert L.sdfk_eval_grid_moments_scratch(17, 17, 17, 0) == scratch(17 ** 3)
    assert L.sdfk_eval_grid_moments_scratch(17, 17, 17, 2000) == scratch(117 * 17)
    assert L.sdfk_eval_grid_moments_scratch(1025, 1025, 1025, 0) <= 8.01 * 1025 ** 3 + 11e6
    assert L.sdfk_eval_grid_moments_scratch(0, 5, 5, 0) == 0


@pytest.mark.parametrize("shape,slab_cells,cells", [((5, 5, 5), 0, 125), ((17, 17, 17), 2000, 117 * 17), ((3, 130, 1), 0, 390)])
def test_both_entries_carve_the_same_scratch_tail(built, shape, slab_cells, cells):
    """After their own heads — moments' two partial arrays (the formula of test_native_argument_checks), occupancy's 32 KB —
    the two entries lay out one tail: the sizes differ by the heads alone. cells: the slab, whole rows."""
    def partials(units):
        return (-(-min(units, 65536) // 4) * 4 * 80 + 255) // 256 * 256
    L = built.lib()
    got = L.sdfk_eval_grid_moments_scratch(*shape, slab_cells) - L.sdfk_eval_grid_occupancy_scratch(*shape, slab_cells)
    assert got == partials(cells) + partials(-(-cells // 1024)) - 32768


def test_new_entries_are_declared_and_exported(built):
    header = open(os.path.join(ROOT, "include", "sdfk.h")).read()
    for name in ("sdfk_eval_grid_moments_scratch", "sdfk_eval_grid_moments"):
        assert name in built.SIGNATURES and hasattr(built.lib(), name) and name + "(" in header
    assert "#define SDFK_FLAVOUR_MOMENTS 14" in header and built.FLAVOUR_MOMENTS == 14
    assert "#define SDFK_ABI_VERSION 1" in header and built.lib().sdfk_abi_version() == 1
    assert callable(built.Program.moments_grid)
    import __graft_entry__
    assert "sdfk_moments.inc" in __graft_entry__.DEPS and "sdfk_momdev.h" in __graft_entry__.DEPS
    embedded = open(os.path.join(ROOT, "aegolius_amd", "csrc", "sdfk_embedded.inc")).read()
    assert "kEmbeddedMomdev" in embedded and "sdfk_mom_sample" in embedded
    init = open(os.path.join(ROOT, "aegolius_amd", "__init__.py")).read()
    assert "moments" not in init


def test_moments_flavour_builds_for_gfx950(built):
    before = None
    for tree, members in ((workloads.cfg2_tree(ns), 0), (workloads.sphere_union(ns, count=300), 300)):
        prog = built.Program.from_lowered(lower_geometry(tree))
        assert prog.chain_members == members                     # the union: the table-driven body
        if before is None:
            before = prog.compile_check()
        size, _ = prog.compile_flavour(built.FLAVOUR_MOMENTS)
        assert size > 5000
        builds = built.jit_stats()[0]
        again, _ = prog.compile_flavour(built.FLAVOUR_MOMENTS)
        assert again == size and built.jit_stats()[0] == builds  # served from the cache: no hiprtc build ran
        with pytest.raises(built.SdfkError):
            prog.compile_flavour(built.FLAVOUR_MOMENTS | built.FLAVOUR_FLAGS)
        with pytest.raises(built.SdfkError):
            prog.compile_flavour(built.FLAVOUR_MOMENTS | built.FLAVOUR_XY)
    cfg2 = built.Program.from_lowered(lower_geometry(workloads.cfg2_tree(ns)))
    assert cfg2.compile_check() == before > 0                    # (the evaluation flavours: this one is not among them)


_NAMES_SCRIPT = """
import sys
sys.path.insert(0, %r)
import aegolius_amd.cores as ns
from aegolius_amd import _engine, workloads
from aegolius_amd._lower import lower_geometry
for tree in (workloads.cfg2_tree(ns), workloads.sphere_union(ns, count=300)):
    _engine.Program.from_lowered(lower_geometry(tree)).compile_flavour(_engine.FLAVOUR_MOMENTS)
"""


def test_moments_flavour_exports_its_kernels(built, tmp_path):
    """The code objects of the flavour, built by a fresh process into an on-disk cache of its own, carry the two kernels
    the launcher asks for by name (and none of the occupancy or ray kernels)."""
    env = dict(os.environ, SDFK_CACHE_DIR=str(tmp_path))
    subprocess.run([sys.executable, "-c", _NAMES_SCRIPT % ROOT], check=True, env=env, timeout=600)
    blobs = [open(os.path.join(str(tmp_path), f), "rb").read() for f in sorted(os.listdir(str(tmp_path))) if f.endswith(".co")]
    assert len(blobs) == 2
    for blob in blobs:
        assert b"sdfk_spec_mom_list" in blob and b"sdfk_spec_mom_all" in blob
        assert b"sdfk_spec_occ_list" not in blob and b"sdfk_spec_rays" not in blob
