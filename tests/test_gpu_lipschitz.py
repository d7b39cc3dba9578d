"""Every kernel that trusts the Lipschitz tables (aegolius_amd/_lipschitz.py), on the catalogue of tests/lipschitz_scenes.py:
the brick, row-block, grid and chain culling kernels return the un-culled kernel's bits, every skip decision of the two
probes is justified point by point by the float64 oracle, no ray of the sphere tracer passes through a surface, and the
occupancy kernel's skipping changes no bit.

The grids (lipschitz_scenes.GRID_3D / GRID_2D) are the smallest on which bricks go wrong: rows of 257 points (bricks
straddle row ends), 24 rows per plane (no multiple of the 16 rows of a row block), a total that is no multiple of 128, and a
device pointer shifted by 3 floats.

A specialised kernel costs a hiprtc build of about a second per flavour, and an entry needs up to nine flavours: the builds
of the tests selected in a session run ahead on a thread pool (two to three minutes for the whole file, where the tests
themselves take one), see `kernels_built_ahead`."""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import aegolius_amd
import aegolius_amd.cores as ns
import lipschitz_scenes as S
import occupancy_reference as occ_ref
import render_reference as ref
import test_gpu_parity as T
from aegolius_amd import _engine, occupancy, render
from aegolius_amd._lower import lower_geometry
from oracle import sdf_oracle

pytestmark = pytest.mark.gpu

MISALIGN = 3
F = _engine
BITS_FLAVOURS = {3: (F.FLAVOUR_PLAIN_ARRAY, F.FLAVOUR_TILE_ARRAY, F.FLAVOUR_ROWS_ARRAY, F.FLAVOUR_TILE_GRID, F.FLAVOUR_ROWS_GRID),
                 2: (F.FLAVOUR_PLAIN_ARRAY, F.FLAVOUR_TILE_ARRAY, F.FLAVOUR_ROWS_ARRAY, F.FLAVOUR_TILE_GRID, F.FLAVOUR_ROWS_GRID,
                     F.FLAVOUR_ROWS2D_ARRAY, F.FLAVOUR_ROWS2D_GRID)}
MASK_FLAVOURS = (F.FLAVOUR_TILE_MASK, F.FLAVOUR_ROWS_MASK)

RAY_ENTRIES = ["leaf:" + n for n in S.LEAVES_3D] + ["pair:" + n for n in S.PAIRS_FOR_RAYS]
OCCUPANCY_ENTRIES = (["leaf:" + n for n in S.LEAVES] + ["pair:" + n for n in S.PAIRS_FOR_RAYS + S.PAIRS_FOR_OCCUPANCY_2D])
W, H = 64, 48


def geometry(entry):
    """-> (geometry, dim) of "leaf:<name>", "pair:<name>" or "chain:<name>"."""
    kind, name = entry.split(":", 1)
    if kind == "leaf":
        return S.LEAVES[name].build(ns), S.LEAVES[name].dim
    if kind == "pair":
        return S.PAIRS[name].tree(ns), S.PAIRS[name].dim
    return S.CHAINS[name].tree(ns), S.CHAINS[name].dim


@pytest.fixture(scope="module")
def engine(built):
    built.require_gpu()
    return built


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    aegolius_amd.config.mode = 0


@pytest.fixture(scope="module", autouse=True)
def kernels_built_ahead(request, engine):
    """The hiprtc builds of the tests selected in this session, sixteen at a time (the build cache is shared by all
    programs of one source, so the tests find their kernels built)."""
    wanted = {"test_culled_kernels_return_the_plain_kernels_bits": lambda dim: BITS_FLAVOURS[dim],
              "test_every_skip_is_justified": lambda dim: MASK_FLAVOURS,
              "test_no_ray_passes_through_a_surface": lambda dim: (F.FLAVOUR_RAYS,),
              "test_occupancy_equals_the_block_sum_of_the_fine_field": lambda dim: (F.FLAVOUR_OCCUPANCY, F.FLAVOUR_PLAIN_GRID)}
    jobs, programs = set(), {}
    for item in request.session.items:
        fn = getattr(item, "originalname", None)
        if item.module is not request.module or fn not in wanted or not hasattr(item, "callspec"):
            continue
        entry = item.callspec.params["entry"]
        if entry.startswith("chain:"):
            continue                                            # chain mode runs on table-driven kernels
        geo, dim = geometry(entry)
        if entry not in programs:
            programs[entry] = engine.Program.from_lowered(lower_geometry(geo))
        jobs |= {(entry, flavour) for flavour in wanted[fn](dim)}

    def build(job):
        try:
            programs[job[0]].compile_flavour(job[1])
        except engine.SdfkError:
            pass                                                # the test that needs the kernel reports it
    with ThreadPoolExecutor(16) as pool:
        list(pool.map(build, sorted(jobs)))
    return len(jobs)


def grid32(dim):
    axes, co = S.grid(dim)
    axes32 = [a.astype(np.float32) for a in axes] + [np.zeros(1, dtype=np.float32)] * (3 - dim)
    return axes32, np.ascontiguousarray(co, dtype=np.float32)


def oracle(geo, co32):
    with np.errstate(all="ignore"):
        return sdf_oracle.evaluate(geo, co32.astype(np.float64))


# ---- bits ---------------------------------------------------------------------------------------------------------------------
BITS_ENTRIES = ["pair:" + n for n in S.PAIRS] + ["chain:" + n for n in S.CHAINS]


@pytest.mark.parametrize("entry", BITS_ENTRIES)
def test_culled_kernels_return_the_plain_kernels_bits(entry, engine):
    geo, dim = geometry(entry)
    low = lower_geometry(geo)
    assert len(low.cull_sites) > 0 and np.isfinite(low.lipschitz)
    prog = engine.Program.from_lowered(low)
    if entry.startswith("chain:"):
        assert prog.chain_members == S.CHAIN_MEMBERS                     # table-driven chain mode
    axes, co32 = grid32(dim)
    n = co32.shape[1]
    row_len = axes[dim - 1].size
    assert n % row_len == 0 and n % 128 != 0 and row_len % 32 != 0
    stride = n + 5
    plain = T._device_eval(engine, prog, co32, n, stride, MISALIGN, engine.MODE_NOCULL)
    got = {"bricks": T._device_eval(engine, prog, co32, n, stride, MISALIGN, engine.MODE_SPECIALIZED),
           "row blocks": T._device_eval(engine, prog, co32, n, stride, MISALIGN, engine.MODE_SPECIALIZED, row_len=row_len),
           "grid": prog.eval_grid_host(axes, mode=engine.MODE_SPECIALIZED)}
    if dim == 2:
        got["flat row blocks"] = T._device_eval(engine, prog, co32, n, stride, MISALIGN, engine.MODE_SPECIALIZED,
                                                row_len=row_len, flat=True)
    else:
        got["row blocks in planes"] = T._device_eval(engine, prog, co32, n, stride, MISALIGN, engine.MODE_SPECIALIZED,
                                                     row_len=row_len, plane_rows=axes[1].size)
    if low.fits_interpreter:
        got["interpreter"] = T._device_eval(engine, prog, co32, n, stride, MISALIGN, engine.MODE_INTERPRET)
    else:
        assert entry.startswith("chain:")
    for name, out in got.items():
        np.testing.assert_array_equal(out, plain, err_msg="%s: %s" % (entry, name))
    s0, cnt = 3 * row_len, (n // row_len - 5) * row_len                 # a slab of whole rows
    np.testing.assert_array_equal(prog.eval_grid_host(axes, s0, cnt, mode=engine.MODE_SPECIALIZED), plain[s0:s0 + cnt])
    T.check(entry, plain, oracle(geo, co32))


# ---- masks --------------------------------------------------------------------------------------------------------------------
def brick_masks(engine, prog, co32):
    """-> (masks (nb,) uint64, brick of every point) of the 128-point line bricks."""
    n = co32.shape[1]
    stride = (n + 255) // 256 * 256
    lib = engine.lib()
    nb = (n + 2047) // 2048 * 16
    d_co, d_m = lib.sdfk_malloc(3 * stride * 4), lib.sdfk_malloc(nb * 8)
    try:
        host = np.zeros((3, stride), dtype=np.float32)
        host[:, :n] = co32
        engine.check(lib.sdfk_memcpy_h2d(ctypes.c_void_p(d_co), host.ctypes.data_as(ctypes.c_void_p), host.nbytes), "h2d")
        engine.check(lib.sdfk_debug_brick_masks(prog.handle, ctypes.c_void_p(d_co), n, stride, ctypes.c_void_p(d_m), None),
                     "masks")
        engine.check(lib.sdfk_sync(None), "sync")
        masks = np.empty(nb, dtype=np.uint64)
        engine.check(lib.sdfk_memcpy_d2h(masks.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(d_m), masks.nbytes), "d2h")
    finally:
        lib.sdfk_free(ctypes.c_void_p(d_co))
        lib.sdfk_free(ctypes.c_void_p(d_m))
    return masks[:(n + 127) // 128], np.arange(n, dtype=np.int64) // 128


def row_masks(engine, prog, co32, L):
    """-> (masks (nb,) uint64 of sites 0-31, brick of every point) of the row blocks (layout: include/sdfk.h)."""
    n = co32.shape[1]
    lib = engine.lib()
    nb, brows = ctypes.c_int64(0), ctypes.c_int(0)
    engine.check(lib.sdfk_debug_row_masks(prog.handle, ctypes.c_void_p(1), n, n, L, None, ctypes.byref(nb), ctypes.byref(brows),
                                          None), "size query")
    nb, brows = nb.value, brows.value
    R = n // L
    nchunk = L // 32 if L % 32 == 0 else (L + 62) // 32
    assert nb == nchunk * ((R + brows - 1) // brows)
    d_co, d_m = lib.sdfk_malloc(3 * n * 4), lib.sdfk_malloc(nb * 24)
    try:
        engine.check(lib.sdfk_memcpy_h2d(ctypes.c_void_p(d_co), co32.ctypes.data_as(ctypes.c_void_p), co32.nbytes), "h2d")
        engine.check(lib.sdfk_debug_row_masks(prog.handle, ctypes.c_void_p(d_co), n, n, L, ctypes.c_void_p(d_m), None, None,
                                              None), "masks")
        engine.check(lib.sdfk_sync(None), "sync")
        words = np.empty((nb, 3), dtype=np.uint64)
        engine.check(lib.sdfk_memcpy_d2h(words.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(d_m), words.nbytes), "d2h")
    finally:
        lib.sdfk_free(ctypes.c_void_p(d_co))
        lib.sdfk_free(ctypes.c_void_p(d_m))
    assert np.all(words[:, 1] == 0)
    r, z = np.divmod(np.arange(n, dtype=np.int64), L)
    brick = (r // brows) * nchunk + ((r * L + z) >> 5) - ((r * L) >> 5)
    assert brick.max() < nb
    return words[:, 0], brick


@pytest.mark.parametrize("entry", ["pair:" + n for n in S.PAIRS])
def test_every_skip_is_justified(entry, engine):
    """Where a probe says that an operand of the pair's site is irrelevant on a brick, the float64 oracle of the whole tree
    equals, at every point of that brick, the oracle of the tree with the kept operand alone under the same outer
    modifications (Pair.kept; a kept second operand of a subtraction enters negated) to 1e-12 max(1, |f|). Where the gap of
    the existing mask tests holds (b - a >= w), the combiners return the other operand exactly, so this is that rule, and
    it also holds the operations above the site to account. No site has both bits set, and in every entry both probes skip
    somewhere and keep both operands somewhere."""
    pair = S.PAIRS[entry.split(":", 1)[1]]
    low = lower_geometry(pair.tree(ns))
    prog = engine.Program.from_lowered(low)
    site = pair.site(ns, lower_geometry)
    assert len(low.cull_sites) <= 32
    axes, co32 = grid32(pair.dim)
    whole = oracle(pair.tree(ns), co32)
    alone = [oracle(pair.kept(ns, which), co32) for which in (0, 1)]
    tol = 1e-12 * np.maximum(1.0, np.abs(whole))
    off = [np.abs(whole - alone[which]) > tol for which in (0, 1)]            # points where operand `which` alone is wrong
    for kind, (masks, brick) in (("bricks", brick_masks(engine, prog, co32)),
                                 ("row blocks", row_masks(engine, prog, co32, axes[pair.dim - 1].size))):
        for k in range(len(low.cull_sites)):
            both = (masks >> np.uint64(2 * k)) & np.uint64(3)
            assert not np.any(both == np.uint64(3)), (entry, kind, k)
        skip_a = ((masks >> np.uint64(2 * site)) & np.uint64(1)).astype(bool)
        skip_b = ((masks >> np.uint64(2 * site + 1)) & np.uint64(1)).astype(bool)
        for skipped, kept, label in ((skip_b, 0, "second"), (skip_a, 1, "first")):
            wrong = np.zeros(masks.size, dtype=bool)
            np.logical_or.at(wrong, brick, off[kept])
            bad = np.flatnonzero(wrong & skipped)
            assert bad.size == 0, "%s, %s: the %s operand is skipped on %d bricks where it matters (first: brick %d)" % (
                entry, kind, label, bad.size, bad[0])
        print("%s, %s: %d of %d bricks skip the first operand, %d the second" % (entry, kind, skip_a.sum(), masks.size,
                                                                                 skip_b.sum()))
        assert np.any(skip_a | skip_b), (entry, kind, "nothing is skipped anywhere")
        assert np.any(~(skip_a | skip_b)), (entry, kind, "no brick keeps both operands")


# ---- rays ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", RAY_ENTRIES)
def test_no_ray_passes_through_a_surface(entry, engine):
    """The two assertions of test_gpu_render.test_soundness_every_ray, for every ray of a 64 x 48 view: hits lie within
    thr + slack of the surface, and f > -slack at 64 samples along every traversed segment. Where the eye itself lies in
    the solid (a half space, the complement of a box) there is no segment to traverse: those rays must hit at t_min."""
    geo, _ = geometry(entry)
    L = lower_geometry(geo).lipschitz
    cam = ref.cameras()["perspective"]
    t_max, max_steps = 8.0, 256
    o64, d64 = cam.rays(W, H)
    o, d = np.asarray(o64, dtype=np.float32), np.asarray(d64, dtype=np.float32)
    eps, cone = cam.footprint(W, H)
    hits = render.cast(geo, o, d, 0.0, t_max, eps, cone, max_steps)
    o64, d64, t = o.astype(np.float64), d.astype(np.float64), hits.t.astype(np.float64)
    hit = hits.status == render.HIT
    thr = ref.threshold(t, float(np.float32(eps)), float(np.float32(cone)))
    f, slack = ref.slack(geo, o64[:, hit] + t[hit] * d64[:, hit], L)
    over = f - (thr[hit] + slack)
    print("%s: L = %.4g, %d hits, %d misses, %d at the step limit; worst f - (thr + slack) at a hit %.3e" % (
        entry, L, hit.sum(), (hits.status == render.MISS).sum(), (hits.status == render.LIMIT).sum(),
        over.max() if over.size else float("nan")))
    assert np.all(over <= 0.0)
    f0, slack0 = ref.slack(geo, o64, L)
    inside = f0 <= -slack0                                              # the ray starts in the solid
    assert np.all(hit[inside] & (t[inside] == 0.0)), entry
    end = np.where(hits.status == render.MISS, t_max, t)
    for s in np.linspace(0.0, 1.0, 64):
        f, slack = ref.slack(geo, o64 + (s * end) * d64, L)
        assert np.all((f > -slack)[~inside]), (entry, s, float((f + slack)[~inside].min()))


# ---- occupancy ----------------------------------------------------------------------------------------------------------------
OCCUPANCY_GRIDS = {3: [np.linspace(-1.1, 1.1, 17)] * 3, 2: [np.linspace(-S.HALF, S.HALF, 65), np.linspace(-S.HALF, S.HALF, 63)]}


@pytest.mark.parametrize("entry", OCCUPANCY_ENTRIES)
def test_occupancy_equals_the_block_sum_of_the_fine_field(entry, engine):
    """The rule of test_gpu_occupancy.test_equal_to_the_block_sum_of_the_fine_field on 17^3 cells (2-D: 65 x 63), k = 2, and
    partial cells <= near_cells < all cells: the skipping that the bound allows happens and changes no bit."""
    geo, dim = geometry(entry)
    axes, k, level = OCCUPANCY_GRIDS[dim], 2, 0.0
    tabs = occ_ref.tables(axes, k)
    prog = engine.Program.from_lowered(lower_geometry(geo))
    values = prog.eval_grid_host(tabs, mode=engine.MODE_NOCULL)
    with np.errstate(invalid="ignore"):
        counts = occ_ref.block_sum(values <= np.float32(level), axes, k)
    K = k ** dim
    occ = occupancy.fractions(geometry(entry)[0], axes, k, level)
    assert occ.fraction.dtype == np.float32 and occ.fraction.shape == counts.shape
    np.testing.assert_array_equal(occ.fraction, (counts / K).astype(np.float32))
    assert occ.inside_samples == int(counts.sum())
    partial = int(np.count_nonzero((counts > 0) & (counts < K)))
    print("%s: %d partially covered cells <= %d near cells < %d cells" % (entry, partial, occ.near_cells, counts.size))
    assert partial <= occ.near_cells < counts.size
