"""CPU (no GPU needed): the host half of aegolius_amd.autodiff — parameter tangents from the shortcut-free lowering, the
structure checks, the refusals and the channel layout — and the default lowering left as it was."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import aegolius_amd.cores as ns
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


def test_design_lists_the_dual_rule_table(built):
    """DESIGN.md §4.10 names the covered and the refused opcodes; both lines equal the table in csrc/sdfk_dualdev.h."""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    covered = re.search(r"^Covered opcodes: `([^`]*)`", text, re.M).group(1).split()
    refused = re.search(r"^Refused opcodes: `([^`]*)`", text, re.M).group(1).split()
    assert covered == ad.dual_opcodes()
    assert refused == [o.name for o in _ops.OPS if o.name not in covered]
