"""CPU (no GPU needed): the host half of aegolius_amd.autodiff — parameter tangents from the shortcut-free lowering, the
structure checks, the refusals and the channel layout — and the default lowering left as it was."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import aegolius_amd.cores as ns
import autodiff_liveness
import autodiff_scenes
import scenes
from aegolius_amd import _ops, autodiff as ad
from aegolius_amd._lower import NeedsStage, lower_geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tangents(builder, primals, argnums=0):
    low, _origin, rows, _chans, _layout = ad.parameter_tangents(builder, primals, argnums)
    return low, rows


def _op_rows(low, name):
    """(instruction index, parameter offset) of every instruction `name`."""
    return [(i, int(low.code[i, 1])) for i in range(low.code.shape[0]) if _ops.OPS[int(low.code[i, 0]) & 255].name == name]


def test_circle_radius_tangent_is_exactly_one(built):
    low, rows = _tangents(lambda r: ns.Circle(r), (1.0,))
    (_, off), = _op_rows(low, "P_CIRCLE")
    assert rows.shape == (1, low.params.size)
    assert rows[0, off] == 1.0
    assert np.count_nonzero(rows) == 1


def test_translation_at_zero_lowers_and_has_the_analytic_row(built):
    def build(x0):
        s = ns.Sphere(0.5)
        s.move((x0, 0, 0))
        return s
    low, rows = _tangents(build, (0.0,))
    (_, off), = _op_rows(low, "XFORM")            # never XLATE, never aliased: the form does not depend on the value
    want = np.zeros(12)
    want[9] = 1.0                                  # c = R^T t, R = I: dc/dx0 = e_x
    np.testing.assert_array_equal(rows[0, off:off + 12], want)
    assert not np.any(np.delete(rows[0], np.arange(off, off + 12)))


def test_scale_at_one_lowers_and_has_the_analytic_rows(built):
    def build(s):
        o = ns.Sphere(0.5)
        o.set_scale(s)
        return o
    low, rows = _tangents(build, (1.0,))
    (_, xoff), = _op_rows(low, "XFORM")
    (_, voff), = _op_rows(low, "VSCALE")
    np.testing.assert_allclose(rows[0, xoff:xoff + 9], (-np.eye(3)).ravel(), atol=1e-9)   # d(1/s) = -1 at s = 1
    assert rows[0, voff] == pytest.approx(1.0, abs=1e-12)


def test_rotation_angle_at_zero_lowers_and_has_the_analytic_rows(built):
    def build(a):
        o = ns.Box(0.5, 0.4, 0.3)
        o.rotate(a, (0, 0, 1))
        return o
    low, rows = _tangents(build, (0.0,))
    (_, off), = _op_rows(low, "XFORM")
    # M = R^T, R = rot_z(a): dM/da at 0 = [[0, 1, 0], [-1, 0, 0], [0, 0, 0]]
    np.testing.assert_allclose(rows[0, off:off + 9], [0, 1, 0, -1, 0, 0, 0, 0, 0], atol=1e-8)


def test_structure_change_raises():
    def ngon(n):
        return ns.NGon(0.5, n)
    with pytest.raises(ad.StructureError, match="argnum 0"):
        ad.parameter_tangents(ngon, (5.0,))

    def instances(n):                              # the host switches to the instancing branch above 2 instances
        b = ns.Box(0.2, 0.2, 0.2)
        b.linear_instancing(n, (-1.0, 0, 0), (1.0, 0, 0))
        return b
    with pytest.raises(ad.StructureError, match="jumps at argnum 0"):
        ad.parameter_tangents(instances, (2.0,))
    ad.parameter_tangents(instances, (4.0,))      # (the count itself enters the parameters smoothly)


def test_point_cloud_and_signed_trees_are_refused(built):
    pts = np.random.default_rng(1).uniform(-1, 1, (3, 20))

    from aegolius_amd.cores.geom_3d import PointCloud3D

    def cloud(r):
        o = PointCloud3D(pts)
        o.rounding(r)
        return o
    low, origin, rows, _, _ = ad.parameter_tangents(cloud, (0.1,))
    with pytest.raises(ad.UnsupportedOpError, match="P_NEAREST3.*PointCloud3D"):
        ad._program(low, origin)

    def signed(r):
        o = ns.Circle(r)
        o.signed((32, 32, 1))
        return o
    with pytest.raises(ad.UnsupportedOpError, match="staged"):
        ad.parameter_tangents(signed, (0.5,))

    low, origin = ad._lower(ns.Braid(1.0, 0.3, 0.1, 1.0), shortcuts=False)
    with pytest.raises(ad.UnsupportedOpError, match="has no dual rule"):
        ad._program(low, origin)


def test_channel_layout():
    primals = (1.0, np.arange(6.0), 2.0)
    chans, layout = ad.channel_layout(primals, 0)
    assert chans == [(0, None)] and layout == [(0, 1, True)]
    chans, layout = ad.channel_layout(primals, (2, 1))
    assert chans == [(2, None)] + [(1, i) for i in range(6)]
    assert layout == [(0, 1, True), (1, 6, False)]
    with pytest.raises(ValueError):
        ad.channel_layout((np.zeros((2, 2)),), 0)


def test_more_than_four_channels_are_the_rows_of_each_channel(built):
    build = autodiff_scenes.SCENES["multi_position_optimization"][0](ns)
    primals = autodiff_scenes.SCENES["multi_position_optimization"][1]
    low, rows = _tangents(build, primals, (0, 1))
    assert rows.shape == (6, low.params.size)
    for c in range(6):
        _l, one = _tangents(lambda x: build(*[(x if j == c // 3 else primals[j]) for j in range(2)]), (primals[c // 3],), 0)
        np.testing.assert_array_equal(one[c % 3], rows[c])


@pytest.mark.parametrize("name", sorted(autodiff_scenes.SCENES))
def test_every_autodiff_scene_has_dual_rules(name, built):
    fn, primals, argnums = autodiff_scenes.SCENES[name]
    low, origin, rows, chans, _ = ad.parameter_tangents(fn(ns), primals, argnums)
    ad._program(low, origin)
    assert rows.shape[0] == len(chans) and np.all(np.isfinite(rows))


def test_dual_rule_table_covers_the_required_opcodes(built):
    have = set(ad.dual_opcodes())
    required = ("MOVC XFORM XLATE LIN3 CSCALE ELONGATE REVOLVE ROT2D AXREV ZEROZ TWIST BEND INFREP FINREP SYMMETRY FOLDX "
                "ROTSYM LININST P_AXIS P_SPHERE P_CYLINDER P_BOX P_TORUS P_CHAINLINK P_ARC3D P_PLANE P_UPLANE P_SEGMENT3 "
                "P_CONE P_ZSLAB P_CIRCLE P_BOX2 P_SEGMENT2 P_RBOX2 P_TRIANGLE2 P_ARC2 P_NGON").split()
    required += [o.name for o in _ops.OPS if o.kind in ("V_V", "V_VV")]
    assert set(required) <= have
    assert "V_FIELD" not in have and "P_NEAREST3" not in have


def test_default_lowering_is_unchanged(built):
    """Every scene of tests/scenes.py lowers, by default, to the bytes it lowered to before the shortcut-free option
    existed (tests/golden/default_lowering_sha256.json)."""
    with open(os.path.join(ROOT, "tests", "golden", "default_lowering_sha256.json")) as f:
        want = json.load(f)
    got = {}
    for name in sorted(scenes.SCENES):
        try:
            low = lower_geometry(scenes.SCENES[name](ns))
        except NeedsStage:
            continue
        h = hashlib.sha256()
        for part in low.key():
            h.update(part if isinstance(part, bytes) else repr(part).encode())
        h.update(repr((low.n_creg, low.n_vreg)).encode())
        got[name] = h.hexdigest()
    assert got == want


def test_every_dual_rule_is_exercised(built):
    """The scenes the GPU tests check against the oracle use every opcode of the dual-rule table: the parameter-mode scenes
    through the shortcut-free lowering, the point-mode scenes through the default one."""
    seen = set()
    for fn, primals, argnums in autodiff_scenes.SCENES.values():
        low, origin, _rows, _c, _l = ad.parameter_tangents(fn(ns), primals, argnums)
        seen |= {_ops.OPS[int(w) & 255].name for w in low.code[:, 0]}
    for fn in autodiff_scenes.POINT_SCENES.values():
        low, origin = ad._lower(fn(ns), shortcuts=True)
        ad._program(low, origin)
        seen |= {_ops.OPS[int(w) & 255].name for w in low.code[:, 0]}
    assert set(ad.dual_opcodes()) - seen == set()


# ---- reach instead of presence: which terms of the rules the scenes checked against the oracle can see -----------------
_OP_LOWERINGS = {}


def _op_lowerings(name):
    """(geometry, liveness in point mode on the default lowering, liveness in parameter mode over (tx, ty, ang, s) on the
    shortcut-free lowering) of one OP_GEOMETRIES entry, computed once."""
    if name not in _OP_LOWERINGS:
        make = autodiff_scenes.OP_GEOMETRIES[name][0]
        geo = make(ns, *autodiff_scenes.OP_DEFAULTS)
        low, origin = ad._lower(geo, shortcuts=True)
        ad._program(low, origin)
        free, origin, rows, _c, _l = ad.parameter_tangents(lambda *p: make(ns, *p), autodiff_scenes.OP_DEFAULTS, (0, 1, 2, 3))
        ad._program(free, origin)
        _OP_LOWERINGS[name] = (geo, autodiff_liveness.liveness(low, point_mode=True), autodiff_liveness.liveness(free, rows))
    return _OP_LOWERINGS[name]


def _emitted(geometries, shortcuts):
    seen = set()
    for geo in geometries:
        low, _origin = ad._lower(geo, shortcuts=shortcuts)
        seen |= {_ops.OPS[int(w) & 255].name for w in low.code[:, 0]}
    return seen


# ops that one of the two lowerings cannot emit: the copy of a frozen register and the folded sign of a positive map exist
# only with the shortcuts on
DEFAULT_LOWERING_ONLY = {"MOVC", "VEXPFLAG"}
SHORTCUT_FREE_ONLY = set()


def test_every_dual_rule_has_live_input_tangents(built):
    """Every rule's input-tangent terms are reached: for each opcode of the table some OP_GEOMETRIES entry that lists it
    as a target feeds it a register whose tangent can be non-zero, in point mode (default lowering) and in parameter mode
    (shortcut-free lowering, the placement as primals). An opcode that one lowering never emits is exempt there."""
    point, param = set(), set()
    for name, (_make, _dim, targets, _regions) in autodiff_scenes.OP_GEOMETRIES.items():
        _geo, in_point, in_param = _op_lowerings(name)
        assert set(targets) <= set(ad.dual_opcodes()), name
        point |= {l.name for l in in_point if l.input} & set(targets)
        param |= {l.name for l in in_param if l.input} & set(targets)
    ops = set(ad.dual_opcodes())
    assert ops - point - SHORTCUT_FREE_ONLY == set()
    assert ops - param - DEFAULT_LOWERING_ONLY == set()
    # the exemptions are what they claim: the other lowering never emits them, in any geometry of these tests
    geos = [_op_lowerings(name)[0] for name in autodiff_scenes.OP_GEOMETRIES]
    geos += [fn(ns)(*primals) for fn, primals, _a in autodiff_scenes.SCENES.values()]
    geos += [fn(ns) for fn in autodiff_scenes.POINT_SCENES.values()]
    assert _emitted(geos, shortcuts=False) & DEFAULT_LOWERING_ONLY == set()
    assert _emitted(geos, shortcuts=True) & SHORTCUT_FREE_ONLY == set()


# parameterised ops whose parameters no scene of SCENES can move, with the reason
NO_PARAMETER_TANGENT = {
    "VEXPFLAG": "only the default lowering emits it; parameter mode differentiates the shortcut-free lowering, where the "
                "pair stays a positive map followed by VSIGN / VHARDBIN (and the rule's tangent is zero by design)",
}


def test_every_parameterised_dual_rule_has_live_parameter_tangents(built):
    """Every rule's parameter-tangent terms are reached: each opcode with parameters has, in some scene of SCENES, a
    non-zero tangent row on its own parameter slice."""
    live = set()
    for fn, primals, argnums in autodiff_scenes.SCENES.values():
        low, _origin, rows, _c, _l = ad.parameter_tangents(fn(ns), primals, argnums)
        live |= {l.name for l in autodiff_liveness.liveness(low, rows) if l.param}
    want = {o for o in ad.dual_opcodes() if _ops.BY_NAME[o].nparams > 0}
    assert set(NO_PARAMETER_TANGENT) <= want and not set(NO_PARAMETER_TANGENT) & live
    assert want - live - set(NO_PARAMETER_TANGENT) == set()


def _label_rows(regions, local):
    """-> [(labels (n,), names)] for each independent branch point of a regions predicate."""
    lab = np.atleast_2d(regions(local))
    names = regions.labels if isinstance(regions.labels[0], tuple) else (regions.labels,)
    assert lab.shape == (len(names), local.shape[1])
    return list(zip(lab, names))


def test_op_geometry_points_reach_every_branch(built):
    """On the points the GPU tests use, every branch of every branching rule holds at least 3 % of the points (a
    condition on the inputs: the constants and the placement of the entries are chosen for it)."""
    from test_gpu_autodiff import _points
    checked = 0
    for name, (_make, dim, _targets, regions) in sorted(autodiff_scenes.OP_GEOMETRIES.items()):
        if regions is None:
            continue
        local = autodiff_scenes.local_coordinates(_op_lowerings(name)[0], _points(seed=15, dim=dim))
        for labels, names in _label_rows(regions, local):
            assert labels.min() >= 0 and labels.max() < len(names), name
            share = np.bincount(labels, minlength=len(names)) / labels.size
            assert np.all(share >= 0.03), "%s: %s" % (name, dict(zip(names, share.round(4))))
            checked += 1
    assert checked >= 40


def test_regions_follow_the_local_coordinates_of_the_lowering(built):
    """local_coordinates is the map the placement's XFORM applies: the labels are taken where the rules branch."""
    from test_gpu_autodiff import _points
    for name in ("box", "triangle"):
        geo, _p, _f = _op_lowerings(name)
        low, _origin = ad._lower(geo, shortcuts=True)
        assert _ops.OPS[int(low.code[0, 0]) & 255].name == "XFORM"
        P = low.params64[int(low.code[0, 1]):][:12]
        co = _points(seed=15, dim=autodiff_scenes.OP_GEOMETRIES[name][1])
        np.testing.assert_allclose(autodiff_scenes.local_coordinates(geo, co), P[:9].reshape(3, 3).dot(co) - P[9:, None],
                                   rtol=0, atol=1e-12)


def test_frame_predicates_follow_the_lowering(built):
    """The predicates that re-apply an earlier modification use the frame the lowering uses. The default lowering folds
    the frame of mirror / linear_instancing into the placement's XFORM, whose x row is then _frame_x of the local
    coordinates; rotational_symmetry's ROT2D turns by the angle / 2 - phase of _rotsym_regions."""
    from test_gpu_autodiff import _points
    co = _points(seed=15)

    def program(name):
        geo = _op_lowerings(name)[0]
        low, _origin = ad._lower(geo, shortcuts=True)
        names = [_ops.OPS[int(w) & 255].name for w in low.code[:, 0]]
        return geo, low, names

    for name, follower, frame in (("mirror_sphere", "FOLDX", autodiff_scenes._MIRROR),
                                  ("lininst_sphere", "LININST", autodiff_scenes._LININST[1:])):
        geo, low, names = program(name)
        assert names[:2] == ["XFORM", follower], names
        P = low.params64[int(low.code[0, 1]):][:12]
        np.testing.assert_allclose(P[:3].dot(co) - P[9],
                                   autodiff_scenes._frame_x(autodiff_scenes.local_coordinates(geo, co), *frame),
                                   rtol=0, atol=1e-12, err_msg=name)
    geo, low, names = program("rotsym_rod")
    assert names[:3] == ["XFORM", "ROT2D", "ROTSYM"], names
    P = low.params64[int(low.code[0, 1]):][:12]
    np.testing.assert_allclose(P[:9].reshape(3, 3).dot(co) - P[9:, None], autodiff_scenes.local_coordinates(geo, co),
                               rtol=0, atol=1e-12)
    h = 2 * np.pi / 3 / 2 - 0.5
    np.testing.assert_allclose(low.params64[int(low.code[1, 1]):][:2], (np.cos(h), np.sin(h)), rtol=0, atol=1e-12)
    np.testing.assert_allclose(low.params64[int(low.code[2, 1]):][:1], (2 * np.pi / 3,), rtol=0, atol=1e-12)


def test_oracle_kink_filter_keeps_the_op_geometries(built):
    """The float64 oracle alone: the kink filter of the GPU comparison keeps at least 90 % of the points of every entry,
    along x, y, z and along the four placement primals."""
    from test_gpu_autodiff import _points, _reference, _spatial_reference
    for name, (make, dim, _targets, _regions) in sorted(autodiff_scenes.OP_GEOMETRIES.items()):
        geo = _op_lowerings(name)[0]
        co = _points(seed=15, dim=dim)
        for ax in range(3):
            _D, keep = _spatial_reference(geo, co, ax)
            assert keep.mean() >= 0.90, "%s axis %d: %.3f kept" % (name, ax, keep.mean())
        for a in range(4):
            _D, keep = _reference(lambda *p: make(ns, *p), autodiff_scenes.OP_DEFAULTS, a, None, co)
            assert keep.mean() >= 0.90, "%s argnum %d: %.3f kept" % (name, a, keep.mean())


def test_design_lists_the_dual_rule_table(built):
    """DESIGN.md §4.10 names the covered and the refused opcodes; both lines equal the table in csrc/sdfk_dualdev.h."""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    covered = re.search(r"^Covered opcodes: `([^`]*)`", text, re.M).group(1).split()
    refused = re.search(r"^Refused opcodes: `([^`]*)`", text, re.M).group(1).split()
    assert covered == ad.dual_opcodes()
    assert refused == [o.name for o in _ops.OPS if o.name not in covered]
