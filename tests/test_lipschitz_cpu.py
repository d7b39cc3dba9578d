"""The Lipschitz tables of the lowering (aegolius_amd/_lipschitz.py) without a GPU: every entry is reached by the catalogue
(tests/lipschitz_scenes.py), below and above a cull site; every claimed bound holds on the float64 oracle, and is tight
enough that an entry wrong by a factor of two cannot pass; what has no bound lowers to inf, gets no cull site and is
refused by the sphere tracer.

The bound is checked with slope quotients |f(p) - f(q)| / |p - q| <= (1 + 1e-6) L. The margin: float64 rounding of values
up to about 10 over a separation of at least 1e-6 stays below 1e-8, and the 575 geometries the bound was first measured on
(the scenes of tests/scenes.py, random primitives and chains of the fuzzers) gave no false alarm under it.
"""
import zlib

import numpy as np
import pytest

import aegolius_amd.cores as ns
import autodiff_scenes
import lipschitz_scenes as S
from aegolius_amd import _lipschitz, _ops, render
from aegolius_amd._lower import lower_geometry
from oracle import sdf_oracle

TABLES = {"C_C": _lipschitz.C_C, "V_C": _lipschitz.V_C, "V_V": _lipschitz.V_V, "V_VV": _lipschitz.V_VV}
FINITE = {name for table in TABLES.values() for name in table}
MARGIN = 1.0 + 1e-6
PAIRS_PER_KIND = 50000            # random pairs, and as many directed ones

# opcodes without a table entry, each with the reason: _lipschitz.factor returns inf for them
NO_BOUND = {
    "TWIST": "the stretch grows with the distance from the axis", "BEND": "the stretch grows with the distance from the axis",
    "INFREP": "jumps at cell boundaries", "FINREP": "jumps at cell boundaries", "ROTSYM": "jumps at sector boundaries",
    "LININST": "jumps between instances", "CURVEINST": "jumps between instances", "CURVEINSTT": "jumps between instances",
    "P_BRAID": "strands picked by angle: jumps", "P_POLYSIGN": "a sign", "P_SHAPESIGN": "a sign", "VSIGN": "a sign",
    "VHARDBIN": "a step", "VEXPFLAG": "a step", "V_FIELD": "a sampled field of an earlier stage",
    "VSIGMOID": "bounded slope, not tracked", "VCAPEXP": "bounded slope, not tracked", "VGAUSS": "bounded slope, not tracked",
    "VSMOOTHRELU": "bounded slope, not tracked", "VSLOWSTART": "bounded slope, not tracked",
    "VMUL": "product of two fields", "BOLTZ": "weights depend on the values", "BOLTZSUB": "weights depend on the values",
}


# ---- reading lowered code ---------------------------------------------------------------------------------------------------
def fields(word):
    word = int(word)
    return _ops.OPS[word & 255], (word >> 8) & 255, (word >> 16) & 255, word >> 24


def emitted(low):
    return {fields(w)[0].name for w in low.code[:, 0]}


def below_sites(low):
    """Opcodes inside an operand range of any cull site."""
    out = set()
    for _, a0, a1, b0, b1 in low.cull_sites.tolist():
        for i in list(range(a0, a1 + 1)) + list(range(b0, b1 + 1)):
            out.add(fields(low.code[i, 0])[0].name)
    return out


def above_site(low, site):
    """Opcodes the site's operands or result pass through outside its operand ranges: the coordinate maps that produce the
    registers the operands start from (followed backwards from the first operand instruction) and the value operations
    that consume the combiner's result (followed forwards)."""
    idx, a0, _, _, b1 = low.cull_sites[site].tolist()
    out = set()
    written, wanted = set(), set()
    for i in range(a0, b1 + 1):                       # coordinate registers read before the ranges write them
        info, dst, src, _ = fields(low.code[i, 0])
        if info.kind in ("C_C", "V_C") and src not in written:
            wanted.add(src)
        if info.kind == "C_C":
            written.add(dst)
    for i in range(a0 - 1, -1, -1):
        info, dst, src, _ = fields(low.code[i, 0])
        if info.kind == "C_C" and dst in wanted:
            out.add(info.name)
            wanted.discard(dst)
            wanted.add(src)
    tainted = {fields(low.code[idx, 0])[1]}
    for i in range(idx + 1, len(low.code)):
        info, dst, src, src2 = fields(low.code[i, 0])
        if (info.kind == "V_V" and src in tainted) or (info.kind == "V_VV" and (src in tainted or src2 in tainted)):
            out.add(info.name)
            tainted.add(dst)
        elif info.kind in ("V_C", "V_V", "V_VV"):
            tainted.discard(dst)
    return out


@pytest.fixture(scope="module")
def lowered(built):
    """name -> LoweredProgram of every LEAVES and PAIRS entry (the point tree of P_NEARTREE is built by the library)."""
    leaves = {n: lower_geometry(l.build(ns)) for n, l in S.LEAVES.items()}
    pairs = {n: lower_geometry(p.tree(ns)) for n, p in S.PAIRS.items()}
    return leaves, pairs


# ---- reach --------------------------------------------------------------------------------------------------------------------
def test_the_tables_have_62_entries_and_every_opcode_is_accounted_for():
    assert len(FINITE) == 62 and sum(len(t) for t in TABLES.values()) == 62
    for kind, table in TABLES.items():
        assert all(_ops.BY_NAME[name].kind == kind for name in table), kind
    names = {o.name for o in _ops.OPS}
    assert FINITE <= names and set(NO_BOUND) <= names
    assert not FINITE & set(NO_BOUND)
    assert names - FINITE - set(NO_BOUND) == set(), "new opcodes need a table entry or a line in NO_BOUND"


def test_every_entry_is_emitted_by_a_leaf_with_a_finite_bound(lowered):
    leaves, _ = lowered
    reached = set()
    for name, low in leaves.items():
        assert np.isfinite(low.lipschitz) and low.lipschitz > 0, name
        ops = emitted(low)
        assert set(S.LEAVES[name].targets) <= ops, (name, sorted(set(S.LEAVES[name].targets) - ops))
        reached |= ops
    assert FINITE - reached == set()
    assert set().union(*(l.targets for l in S.LEAVES.values())) == FINITE


def test_every_entry_lies_below_a_cull_site_of_a_pair(lowered):
    _, pairs = lowered
    below = set()
    for name, low in pairs.items():
        pair = S.PAIRS[name]
        assert np.isfinite(low.lipschitz), name
        site = pair.site(ns, lower_geometry)
        assert len(low.cull_sites) > site, name
        idx = int(low.cull_sites[site, 0])
        assert fields(low.code[idx, 0])[0].name == pair.code, name
        if pair.outer is None:
            # the operand range of the leaf holds what the leaf was built for
            lo, hi = (1, 2) if pair.leaf_first else (3, 4)
            inside = {fields(low.code[i, 0])[0].name
                      for i in range(int(low.cull_sites[site, lo]), int(low.cull_sites[site, hi]) + 1)}
            assert set(S.LEAVES[pair.leaf].targets) <= inside, (name, sorted(set(S.LEAVES[pair.leaf].targets) - inside))
        below |= below_sites(low)
    assert FINITE - below == set()


def test_every_map_and_value_operation_lies_above_a_cull_site_of_a_pair(lowered):
    _, pairs = lowered
    above = set()
    for name, pair in S.PAIRS.items():
        if pair.outer is None:
            continue
        got = above_site(pairs[name], pair.site(ns, lower_geometry))
        assert set(pair.targets) <= got, (name, sorted(set(pair.targets) - got))
        above |= got
    wanted = set(TABLES["C_C"]) | set(TABLES["V_V"]) | set(TABLES["V_VV"])
    assert wanted - above == set()


def test_a_coordinate_map_above_a_site_is_carried_by_its_k(lowered):
    """K = L_a + L_b of a site is taken with respect to the ROOT point: a contraction above the site (the field shrinks by
    0.6, coordinates grow by 1 / 0.6) multiplies it."""
    _, pairs = lowered
    k = lambda name: float(pairs[name].cull_k[0])                     # noqa: E731
    assert abs(k("smin3_a_box") - 2.0) <= 1e-6
    assert abs(k("above_cscale") - 2.0 / 0.6) <= 1e-6 and abs(k("above_cscale_grow") - 2.0 / 1.7) <= 1e-6
    assert abs(k("above_xform") - 2.0 / 0.6) <= 1e-6
    s = np.tan(0.8)
    assert abs(k("above_lin3") - (s + np.sqrt(s * s + 4.0))) <= 1e-5
    assert abs(k("above_vlinfall") - 2.0) <= 1e-6                     # a value map above the site does not enter


# ---- the bound ----------------------------------------------------------------------------------------------------------------
def _seed(*parts):
    return zlib.crc32(" ".join(parts).encode())


def sample_pairs(name, dim, frames, count=PAIRS_PER_KIND):
    """-> p, q (3, 2 count): `count` random pairs with |p - q| log-uniform in [1e-6, 1e-2] inside the test domain, and as
    many directed ones whose midpoints lie within 1e-3 of a coordinate plane, a coordinate axis or the origin of one of
    `frames` (placed geometries: autodiff_scenes.world_coordinates), half of them pointing across it."""
    rng = np.random.default_rng(_seed("pairs", name))
    n = 2 * count
    mid = rng.uniform(-S.HALF + 0.01, S.HALF - 0.01, (3, n))
    d = rng.normal(size=(3, n))
    h = 10.0 ** rng.uniform(-6.0, -2.0, n)
    # directed: local midpoints with one, two or three coordinates within 1e-3 (in world units) of zero
    local = rng.uniform(-1.0, 1.0, (3, count))
    small = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 1, 1], [1, 0, 1], [1, 1, 0], [1, 1, 1]], dtype=bool)
    which = small[rng.integers(0, len(small), count)].T                        # (3, count)
    across = rng.random(count) < 0.5
    per = (count + len(frames) - 1) // len(frames)
    for k, geo in enumerate(frames):
        sl = slice(k * per, min((k + 1) * per, count))
        m = sl.stop - sl.start
        if m <= 0:
            break
        scale = abs(float(geo.scale))
        R = np.asarray(geo.rotation_matrix, dtype=np.float64)
        off = rng.uniform(-1e-3, 1e-3, (3, m)) / (np.sqrt(3.0) * max(scale, 1e-12))
        loc = np.where(which[:, sl], off, local[:, sl])
        mid[:, count + sl.start:count + sl.stop] = autodiff_scenes.world_coordinates(geo, loc)
        dl = rng.normal(size=(3, m))
        dl = np.where(across[sl] & ~which[:, sl], 0.0, dl)                      # across: along the small coordinates only
        d[:, count + sl.start:count + sl.stop] = R.dot(dl)
    if dim == 2:
        mid[2] = 0.0
        d[2] = 0.0
    norm = np.linalg.norm(d, axis=0)
    d = np.where(norm > 0, d / np.where(norm > 0, norm, 1.0), np.array([[1.0], [0.0], [0.0]]))
    return mid - 0.5 * h * d, mid + 0.5 * h * d


def evaluate(geometry, co, chunk=40000):
    with np.errstate(all="ignore"):
        return np.concatenate([sdf_oracle.evaluate(geometry, co[:, i:i + chunk]) for i in range(0, co.shape[1], chunk)])


def quotients(build, p, q):
    fp, fq = evaluate(build(), p), evaluate(build(), q)
    assert np.all(np.isfinite(fp)) and np.all(np.isfinite(fq))
    return np.abs(fp - fq) / np.linalg.norm(p - q, axis=0)


def check_bound(name, build, dim, frames):
    L = lower_geometry(build()).lipschitz
    assert np.isfinite(L) and L > 0, name
    p, q = sample_pairs(name, dim, frames)
    separation = np.linalg.norm(p - q, axis=0)
    assert separation.min() >= 1e-6 * (1 - 1e-9) and separation.max() <= 1e-2 * (1 + 1e-9)
    ratio = quotients(build, p, q) / L
    worst = int(np.argmax(ratio))
    assert ratio[worst] <= MARGIN, "%s: slope %.6g L at p = %r (|p - q| = %.3g, L = %.6g); %.3g of the pairs exceed" % (
        name, ratio[worst], p[:, worst].tolist(), separation[worst], L, float((ratio > MARGIN).mean()))
    return float(ratio[worst])


# Leaves whose largest quotient stays below 0.9 L, with the measured ratio and the reason: loose by construction.
LOOSE = {
    "extrude_circle": (0.7071, "EXTRUDE claims sqrt(2) max(a, b) for max(a, b) and |(max(a, 0), max(b, 0))| together; the "
                               "extruded circle and the slab have orthogonal gradients, so 1 is reached, not sqrt(2)"),
}
# The sums (VADD / VDIFF: L_a + L_b) are tight only where the two gradients are parallel: reached to 0.93 - 0.998 here.
NOT_VACUOUS, TIGHT = 0.5, 0.9


@pytest.mark.parametrize("name", sorted(S.LEAVES))
def test_leaf_bound_holds_and_is_not_vacuous(name):
    leaf = S.LEAVES[name]
    worst = check_bound(name, lambda: leaf.build(ns), leaf.dim, [leaf.build(ns)])
    assert worst >= NOT_VACUOUS, "%s: the largest quotient is %.4f L: a bound twice too large would pass" % (name, worst)
    if name in LOOSE:
        assert abs(worst - LOOSE[name][0]) <= 0.02, (name, worst)
    else:
        assert worst >= TIGHT, (name, worst)


@pytest.mark.parametrize("leaf_name", sorted(S.LEAVES))
def test_pair_bounds_hold(leaf_name):
    """Every PAIRS entry of one leaf (as A and as B under the seven combiners)."""
    for name, pair in S.PAIRS.items():
        if pair.leaf == leaf_name and pair.outer is None:
            check_bound(name, lambda: pair.tree(ns), pair.dim, [pair.placed_leaf(ns)])


@pytest.mark.parametrize("name", sorted(n for n, p in S.PAIRS.items() if p.outer is not None))
def test_pair_bounds_hold_under_an_operation_above_the_site(name):
    pair = S.PAIRS[name]
    check_bound(name, lambda: pair.tree(ns), pair.dim, [pair.placed_leaf(ns)])


@pytest.mark.parametrize("name", sorted(S.CHAINS))
def test_chain_bound_holds(name):
    chain = S.CHAINS[name]
    low = lower_geometry(chain.tree(ns))
    assert len(chain.member_names()) == S.CHAIN_MEMBERS >= 22 and len(low.cull_sites) >= S.CHAIN_MEMBERS - 1
    check_bound(name, lambda: chain.tree(ns), chain.dim, chain.members(ns))


# leaves with a combiner of their own: as a member they keep a combination out of chain mode, PAIRS covers them
NOT_IN_CHAINS = {"segmented_line3_closed", "movc_displacement_in_union", "alias_symmetry_in_child", "pair_vmin", "pair_vmax",
                 "pair_vsubtract", "pair_smin2", "pair_smin3", "pair_smax3", "pair_ssub3"}


def test_every_leaf_without_a_combiner_is_a_member_of_a_chain():
    members = set()
    for chain in S.CHAINS.values():
        members |= set(chain.member_names())
    assert members == set(S.LEAVES) - NOT_IN_CHAINS
    for name in NOT_IN_CHAINS:
        assert len(lower_geometry(S.LEAVES[name].build(ns)).cull_sites) > 0 or name == "segmented_line3_closed"


# ---- placement of the pairs -------------------------------------------------------------------------------------------------
def emulated_bricks(dim, co):
    """Centres and radii of the bricks of the two culling kernels on a grid of the GPU tests, to first order: line bricks
    are 128 consecutive points, row blocks 32 points of 16 consecutive rows. -> {kind: (member (n,), centre (3, nb), rho)}.
    (The kernels split and bound their bricks more finely; the GPU tests read their real decisions.)"""
    shape = (S.GRID_3D if dim == 3 else S.GRID_2D)[0]
    n, L = co.shape[1], shape[-1]
    flat = np.arange(n)
    member = {"line": flat // 128, "row": (flat // L // 16) * ((L + 31) // 32) + (flat % L) // 32}
    out = {}
    for kind, m in member.items():
        _, m = np.unique(m, return_inverse=True)
        nb = int(m.max()) + 1
        lo, hi = np.full((3, nb), np.inf), np.full((3, nb), -np.inf)
        for a in range(3):
            np.minimum.at(lo[a], m, co[a])
            np.maximum.at(hi[a], m, co[a])
        centre = 0.5 * (lo + hi)
        out[kind] = (m, centre, np.linalg.norm(0.5 * (hi - lo), axis=0))
    return out


@pytest.mark.parametrize("leaf_name", sorted(S.LEAVES))
def test_pairs_are_placed_where_culling_has_something_to_decide(leaf_name):
    """On the grids of the GPU tests every pair has bricks on which both operands must be kept (the oracle's gap b - a, a + b
    for a subtraction, changes sign inside the brick) and bricks on which one can be skipped with room to spare
    (|gap(c)| >= w + 1.25 K rho at the centre), for line bricks and for row blocks: the GPU test that asks for both kinds of
    decision in every entry is not asking for luck."""
    leaf = S.LEAVES[leaf_name]
    _, co = S.grid(leaf.dim)
    bricks = emulated_bricks(leaf.dim, co)
    for name, pair in S.PAIRS.items():
        if pair.leaf != leaf_name:
            continue
        a, b = (evaluate(g, co) for g in pair.members(ns))
        if pair.outer is not None:
            continue                                             # (a map above the site moves the members: see the GPU test)
        gap = a + b if pair.code in S.SUBTRACTIONS else b - a
        k = float(lower_geometry(pair.tree(ns)).cull_k[pair.site(ns, lower_geometry)])
        for kind, (member, centre, rho) in bricks.items():
            nb = rho.size
            lo, hi = np.full(nb, np.inf), np.full(nb, -np.inf)
            np.minimum.at(lo, member, gap)
            np.maximum.at(hi, member, gap)
            assert np.any((lo < 0.0) & (hi > 0.0)), (name, kind)
            ga, gb = (evaluate(g, centre) for g in pair.members(ns))
            at_centre = np.abs(ga + gb if pair.code in S.SUBTRACTIONS else gb - ga)
            room = at_centre - ((pair.width or 0.0) + 1.25 * k * rho)
            assert np.any(room >= 0.0), (name, kind, float(room.max()), k)


# ---- no bound -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.UNBOUNDED))
def test_unbounded_geometries_lower_to_inf_and_get_no_cull_site(name):
    build, _ = S.UNBOUNDED[name]
    assert lower_geometry(build(ns)).lipschitz == np.inf
    for first in (True, False):
        members = (build(ns), ns.Circle(0.3)) if first else (ns.Circle(0.3), build(ns))
        for code, (operation, width) in S.COMBINERS.items():
            low = lower_geometry(S.combine(ns, operation, width, *members))
            assert low.lipschitz == np.inf and len(low.cull_sites) == 0, (name, code)
    # a bounded pair beside it keeps its own site; the combiner across the unbounded member gets none
    inner = ns.CombineGeometry("UNION2").combine(ns.Circle(0.3), ns.Rectangle(0.4, 0.2))
    low = lower_geometry(ns.CombineGeometry("UNION2").combine(inner, build(ns)))
    assert fields(low.code[-1, 0])[0].name == "VMIN"                  # the combiner across the unbounded member, last
    assert len(low.cull_sites) == 1 and int(low.cull_sites[0, 0]) < len(low.code) - 1


@pytest.mark.parametrize("name", sorted(S.UNBOUNDED))
def test_the_tracer_refuses_unbounded_geometries_without_an_explicit_bound(name, built):
    build, _ = S.UNBOUNDED[name]
    o = np.zeros((3, 4))
    d = np.tile(np.array([[1.0], [0.0], [0.0]]), (1, 4))
    with pytest.raises(ValueError, match=r"instruction \d+ \(\w+, from .*\) has no finite Lipschitz bound.*lipschitz="):
        render.cast(build(ns), o, d)
    with pytest.raises(ValueError, match="lipschitz="):
        render.cast(S.union_with_circle(ns, build(ns)), o, d)
    low, first = render.lower(build(ns))
    assert first is not None and render._bound(low, first, 7.5) == 7.5


# ---- the findings -------------------------------------------------------------------------------------------------------------
def test_neu_circle_of_order_below_one_has_no_bound():
    """Regression. _lipschitz._neucircle claimed 2^(1/order - 1/2) for every order < 2; for order < 1, |x|^order has
    unbounded slope at the axes. Measured on NEUCircle(0.6, order) before the fix (claim / largest quotient):
    0.75: 1.78 / 11.2; 0.5: 2.83 / 136; 0.3: 7.13 / 1093 — and UNION(NEUCircle(0.6, 0.5), Circle(0.3)) had a cull site with
    K = 3.83."""
    for order, claimed in ((0.75, 1.78), (0.5, 2.83), (0.3, 7.13)):
        p, q = sample_pairs("neu %r" % order, 2, [ns.NEUCircle(0.6, order)])
        slope = quotients(lambda: ns.NEUCircle(0.6, order), p, q).max()
        assert abs(2.0 ** (1.0 / order - 0.5) - claimed) < 0.01 and slope > 3.0 * claimed
        L = lower_geometry(ns.NEUCircle(0.6, order)).lipschitz
        assert slope <= MARGIN * L                                     # holds only because L is inf
        assert L == np.inf
    low = lower_geometry(S.union_with_circle(ns, ns.NEUCircle(0.6, 0.5)))
    assert len(low.cull_sites) == 0 and low.lipschitz == np.inf
    for order, want in ((1.0, np.sqrt(2.0)), (1.5, 2.0 ** (1 / 1.5 - 0.5)), (1.999, 2.0 ** (1 / 1.999 - 0.5)), (2.0, 1.0),
                        (7.5, 1.0), (np.inf, 1.0), (-np.inf, 1.0)):
        assert abs(lower_geometry(ns.NEUCircle(0.6, order)).lipschitz - want) <= 1e-12, order
    low = lower_geometry(S.union_with_circle(ns, ns.NEUCircle(0.6, 1.0)))
    assert len(low.cull_sites) == 1 and abs(float(low.cull_k[0]) - (1.0 + np.sqrt(2.0))) <= 1e-6


def test_a_bent_quad_has_no_bound():
    """Regression. P_QUAD3 claimed 1 for every quad; the field of four vertices that are not coplanar jumps across the
    faces of the prism over the quad (quotients above 1000 on the quad below). Planar quads keep the bound 1."""
    bent = lambda: ns.Quad((-0.6, -0.5, 0.0), (0.6, -0.6, 0.3), (0.7, 0.5, 0.0), (-0.5, 0.6, 0.0))      # noqa: E731
    p, q = sample_pairs("bent quad", 3, [bent()])
    assert quotients(bent, p, q).max() > 100.0
    assert lower_geometry(bent()).lipschitz == np.inf
    assert len(lower_geometry(ns.CombineGeometry("UNION2").combine(bent(), ns.Sphere(0.3))).cull_sites) == 0
    planar = ns.Quad((-0.6, -0.5, 0.0), (0.6, -0.6, 0.2), (0.7, 0.5, 0.0), (-0.5, 0.6, -0.2))            # tests/scenes.py
    planar.rotate(0.7, (0.3, -0.5, 0.8))
    assert lower_geometry(planar).lipschitz == 1.0
