"""Geometries for the tests of the Lipschitz bookkeeping (aegolius_amd/_lipschitz.py, tracked in _lower.py) and of every
kernel that trusts it: brick / row-block / grid / chain culling, the sphere tracer's step f / L and the occupancy
kernel's skipping.

Builders only, every one takes `ns` (the layout of aegolius_amd.cores), so that the same text drives the lowering and the
float64 oracle. Parameters and placements are drawn from a generator seeded by the entry's name: an entry is the same
geometry every time it is built.

LEAVES     name -> Leaf: one geometry per entry of the four tables C_C / V_C / V_V / V_VV (and the parameter ranges and
           instruction folds named in the module text below), placed by a random rigid motion
PAIRS      name -> Pair: combine(A, B) with a cull site at the top; every leaf as A and as B against a plain sphere
           (circle) under every CULLABLE combiner, and every C_C / V_V / V_VV operation applied ABOVE such a site
CHAINS     name -> Chain: hard unions / intersections of 24 members that cycle through LEAVES (table-driven chain mode)
UNBOUNDED  name -> builder: geometries whose bound must be infinite
"""
import zlib

import numpy as np

HALF = 1.2                     # the CPU tests sample [-HALF, HALF]^3 (2-D entries: z = 0)
# The grids of the GPU tests: (points per axis, (lo, hi) per axis), rows along the last axis. A line brick is 128 consecutive
# points and a row block 32 points of 16 rows: on grids this small they are large against the geometry, so the grids are
# slabs, long along the axis on which a pair's two members sit (x in 3-D, where a brick has no extent; y in 2-D) and thin
# along the others: brick radii of about 0.2 (3-D), 0.16 (2-D row blocks) and 0.46 (2-D line bricks).
GRID_3D = ((9, 24, 257), ((-1.2, 1.2), (-0.3, 0.3), (-0.4, 0.4)))
GRID_2D = ((40, 333), ((-0.3, 0.3), (-1.2, 1.2)))
# where the members of a pair go on those grids: the leaf is moved by LEAF_SHIFT, the partner sits around PARTNER
LEAF_SHIFT = {3: (-0.5, 0.0, 0.0), 2: (0.0, -0.6, 0.0)}
PARTNER = {3: (0.7, 0.0, 0.0), 2: (0.0, 0.95, 0.0)}
PARTNER_SUBTRACTED = {3: (-0.2, 0.0, 0.0), 2: (0.0, -0.3, 0.0)}      # a subtraction decides where the two members overlap
PARTNER_RADIUS = 0.4
# (leaf, "compare" | "subtract") -> partner centre (and radius), for the leaves on which the default leaves a kernel nothing
# to skip or nothing to keep (test_lipschitz_cpu.test_pairs_are_placed_where_culling_has_something_to_decide checks every entry)
PARTNER_AT = {
    ('sphere', 'compare'): (0.7, 0.12, 0.0),
    ('sphere_moved', 'compare'): (1.0, 0.0, 0.0),
    ('sphere_shrunk', 'compare'): (1.2, -0.22, 0.0),
    ('box_grown', 'subtract'): (-0.8, 0.0, 0.0),
    ('arc3d', 'subtract'): (-0.6, 0.22, 0.0),
    ('oriented_plane', 'compare'): (0.2, 0.0, 0.0),
    ('segment3', 'subtract'): (-0.4, 0.0, 0.0),
    ('solid_angle', 'compare'): (1.0, 0.0, 0.0),
    ('solid_angle', 'subtract'): (-0.4, 0.0, 0.0),
    ('point_cloud3', 'compare'): (0.7, -0.12, 0.0),
    ('circle', 'compare'): (0.0, 1.2, 0.0),
    ('segment2', 'subtract'): (0.0, -0.5, 0.0),
    ('triangle2', 'compare'): (0.0, 1.2, 0.0),
    ('triangle2', 'subtract'): (0.0, -0.5, 0.0),
    ('arc2', 'subtract'): (0.22, -0.3, 0.0),
    ('sector', 'compare'): (0.12, 1.2, 0.0),
    ('sector', 'subtract'): (0.0, -0.5, 0.0),
    ('infinite_sector', 'compare'): (-0.12, 1.2, 0.0),
    ('infinite_sector', 'subtract'): (0.22, -0.3, 0.0),
    ('ngon_17', 'subtract'): (0.0, -0.5, 0.0),
    ('segmented_line2', 'compare'): (0.0, 1.2, 0.0),
    ('point_cloud2', 'compare'): (0.0, 1.2, 0.0),
    ('point_cloud2', 'subtract'): (0.0, -0.5, 0.0),
    ('neu_circle_1', 'compare'): (0.0, 1.2, 0.0),
    ('neu_circle_inf', 'subtract'): (0.0, -0.7, 0.0),
    ('neu_circle_minf', 'subtract'): (0.0, -0.7, 0.0),
    ('xform_sheared_stretch', 'subtract'): (-0.2, -0.22, 0.0),
    ('cscale_negative', 'compare'): (0.4, 0.0, 0.0),
    ('cscale_negative', 'subtract'): (-0.8, -0.12, 0.0),
    ('extrude_circle', 'compare'): (1.0, 0.0, 0.0),
    ('symmetry_x', 'compare'): (0.7, 0.12, 0.0),
    ('symmetry_y', 'subtract'): (-0.2, -0.12, 0.0),
    ('mirror', 'subtract'): (-0.2, 0.12, 0.0),
    ('vaffine_shrink', 'compare'): (0.7, 0.12, 0.0),
    ('vneg', 'compare'): (0.2, 0.0, 0.0),
    ('vneg', 'subtract'): (0.2, 0.0, 0.0),
    ('vonion', 'compare'): (0.7, 0.22, 0.0),
    ('vconcentric', 'compare'): (0.7, -0.12, 0.0),
    ('vlinfall_steep', 'compare'): (1.0, 0.0, 0.0),
    ('vlinfall_steep', 'subtract'): (0.0, 0.0, 0.0),
    ('vlinfall_flat', 'subtract'): (-0.2, 0.0, 0.0, 0.8),
    ('vlinfall_mixed', 'compare'): (1.0, 0.0, 0.0),
    ('vlinfall_mixed', 'subtract'): (-0.2, -0.22, 0.0, 2.0),
    ('pair_vadd', 'subtract'): (-0.2, -0.12, 0.0),
    ('pair_smin2', 'compare'): (1.0, -0.12, 0.0),
    ('pair_smax3', 'compare'): (0.7, 0.12, 0.0),
    ('pair_smax3', 'subtract'): (-0.6, 0.0, 0.0),
    ('pair_ssub3', 'compare'): (0.4, 0.22, 0.0),
}
SKEW_AXIS = (0.3, -0.5, 0.8)

LEAVES, PAIRS, CHAINS, UNBOUNDED = {}, {}, {}, {}

# CULLABLE opcode -> (operation name of CombineGeometry, width or None)
COMBINERS = {"VMIN": ("UNION2", None), "VMAX": ("INTERSECT2", None), "VSUBTRACT": ("SUBTRACT2", None),
             "SMIN2": ("SMOOTH_UNION2_2", 0.12), "SMIN3": ("SMOOTH_UNION2", 0.12), "SMAX3": ("SMOOTH_INTERSECT2", 0.12),
             "SSUB3": ("SMOOTH_SUBTRACT2", 0.12)}
SUBTRACTIONS = ("VSUBTRACT", "SSUB3")


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def combine(ns, operation, width, *members):
    g = ns.CombineGeometry(operation)
    return g.combine(*members) if width is None else g.combine_parametric(*members, parameters=width)


class Leaf:
    """build(ns) -> the placed geometry. dim: 2 when the field does not depend on z. targets: the opcodes the entry
    exists for. The placement (rotate, move, set_scale) is applied last, so that autodiff_scenes.local_coordinates gives
    the leaf's own frame."""

    def __init__(self, name, dim, targets, fn, rigid):
        self.name, self.dim, self.targets, self._fn, self.rigid = name, dim, tuple(targets.split()), fn, rigid

    def build(self, ns):
        r = _rng(self.name)
        o = self._fn(ns, r)
        if self.rigid == "none":
            return o
        if self.rigid != "move":
            axis = r.normal(size=3) if self.dim == 3 else (0.0, 0.0, 1.0)
            o.rotate(r.uniform(-np.pi, np.pi), tuple(axis))
        t = r.uniform(-0.25, 0.25, 3)
        o.move((t[0], t[1], t[2] if self.dim == 3 else 0.0))
        if self.rigid not in ("move", "rotate"):
            o.set_scale(float(self.rigid))
        return o


def leaf(name, dim, targets, rigid="rotate"):
    """rigid: "rotate" (rotation + translation: XFORM), "move" (XLATE), "none", or a scale factor (XFORM + VSCALE)."""
    def deco(fn):
        assert name not in LEAVES, name
        LEAVES[name] = Leaf(name, dim, targets, fn, rigid)
        return fn
    return deco


def _u(r, lo, hi):
    return float(r.uniform(lo, hi))


def shift(o, vector):
    """Move the placed geometry `o` by `vector` in world units (its centre is multiplied by its scale)."""
    o.move(tuple(np.asarray(vector, dtype=np.float64) / float(o.scale)))
    return o


# ---- V_C: one entry per primitive ---------------------------------------------------------------------------------------
leaf("axis_x", 3, "P_AXIS")(lambda ns, r: ns.X(_u(r, -0.3, 0.3)))
leaf("axis_z", 3, "P_AXIS")(lambda ns, r: ns.Z(_u(r, -0.3, 0.3)))
leaf("sphere", 3, "P_SPHERE XFORM")(lambda ns, r: ns.Sphere(_u(r, 0.3, 0.6)))
leaf("sphere_moved", 3, "P_SPHERE XLATE", rigid="move")(lambda ns, r: ns.Sphere(_u(r, 0.3, 0.6)))
leaf("sphere_shrunk", 3, "XFORM VSCALE", rigid=0.45)(lambda ns, r: ns.Sphere(_u(r, 0.6, 1.0)))
leaf("box_grown", 3, "XFORM VSCALE", rigid=2.3)(lambda ns, r: ns.Box(_u(r, 0.2, 0.4), _u(r, 0.15, 0.3), _u(r, 0.1, 0.3)))
leaf("cylinder", 3, "P_CYLINDER")(lambda ns, r: ns.Cylinder(_u(r, 0.2, 0.5), _u(r, 0.4, 1.0)))
leaf("box", 3, "P_BOX")(lambda ns, r: ns.Box(_u(r, 0.4, 1.0), _u(r, 0.3, 0.8), _u(r, 0.2, 0.6)))
leaf("torus", 3, "P_TORUS")(lambda ns, r: ns.Torus(_u(r, 0.4, 0.6), _u(r, 0.08, 0.2)))
leaf("chainlink", 3, "P_CHAINLINK")(lambda ns, r: ns.ChainLink(_u(r, 0.25, 0.4), _u(r, 0.06, 0.12), _u(r, 0.4, 0.8)))
leaf("arc3d", 3, "P_ARC3D")(lambda ns, r: ns.Arc3D(_u(r, 0.5, 0.7), _u(r, 0.08, 0.15), _u(r, 0.1, 0.5), _u(r, 2.0, 2.8)))
leaf("oriented_plane", 3, "P_PLANE")(lambda ns, r: ns.OrientedPlane(tuple(r.normal(size=3)), _u(r, -0.2, 0.2)))
leaf("plane_slab", 3, "P_UPLANE")(lambda ns, r: ns.Plane(tuple(r.normal(size=3)), _u(r, 0.2, 0.5)))
leaf("segment3", 3, "P_SEGMENT3")(lambda ns, r: ns.Line(tuple(r.uniform(-0.6, 0.0, 3)), tuple(r.uniform(0.1, 0.6, 3))))
leaf("cone", 3, "P_CONE")(lambda ns, r: ns.Cone(_u(r, 0.5, 0.9), _u(r, np.pi / 8, np.pi / 4)))
leaf("infinite_cone", 3, "P_INFCONE")(lambda ns, r: ns.InfiniteCone(_u(r, np.pi / 7, np.pi / 4)))
leaf("oriented_infinite_cone", 3, "P_INFCONE")(lambda ns, r: ns.OrientedInfiniteCone(_u(r, np.pi / 7, np.pi / 4)))
leaf("solid_angle", 3, "P_SOLIDANGLE")(
    lambda ns, r: ns.geom_3d.SolidAngle(_u(r, 0.6, 0.9), _u(r, 0.1, 0.4), _u(r, 1.2, 1.8)))
leaf("triangle3", 3, "P_TRIANGLE3")(lambda ns, r: ns.Triangle3D(
    (-0.5, -0.4, _u(r, -0.2, 0.2)), (0.7, -0.2, _u(r, -0.3, 0.3)), (0.1, 0.8, _u(r, -0.4, 0.4))))
leaf("quad3", 3, "P_QUAD3")(lambda ns, r: ns.Quad(                  # planar: a bent quad is in UNBOUNDED
    (-0.6, _u(r, -0.6, -0.4), 0.0), (0.6, -0.6, 0.0), (_u(r, 0.5, 0.8), 0.5, 0.0), (-0.5, _u(r, 0.4, 0.7), 0.0)))
leaf("segmented_line3_closed", 3, "P_SEGLINE3 P_SEGMENT3 VMIN")(
    lambda ns, r: ns.SegmentedLine3D(r.uniform(-0.8, 0.8, (3, 5)), closed=True))
leaf("point_cloud3", 3, "P_NEAREST3")(lambda ns, r: ns.geom_3d.PointCloud3D(r.uniform(-0.8, 0.8, (3, 37))))
leaf("point_cloud3_tree", 3, "P_NEARTREE")(lambda ns, r: ns.geom_3d.PointCloud3D(r.uniform(-0.8, 0.8, (3, 260))))
leaf("circle", 2, "P_CIRCLE")(lambda ns, r: ns.Circle(_u(r, 0.3, 0.6)))
leaf("rectangle", 2, "P_BOX2")(lambda ns, r: ns.Rectangle(_u(r, 0.5, 1.0), _u(r, 0.3, 0.7)))
leaf("segment2", 2, "P_SEGMENT2")(lambda ns, r: ns.Segment((-0.5, _u(r, -0.4, 0.0), 0.0), (0.4, _u(r, 0.0, 0.4), 0.0)))
leaf("rounded_rectangle", 2, "P_RBOX2")(lambda ns, r: ns.RoundedRectangle(
    _u(r, 0.8, 1.0), _u(r, 0.6, 0.8), (_u(r, 0.0, 0.2), 0.05, _u(r, 0.1, 0.25), 0.0)))
leaf("triangle2", 2, "P_TRIANGLE2")(lambda ns, r: ns.Triangle(
    (-0.7, _u(r, -0.6, -0.3), 0.0), (0.7, _u(r, -0.5, -0.2), 0.0), (_u(r, -0.3, 0.3), 0.7, 0.0)))
leaf("arc2", 2, "P_ARC2")(lambda ns, r: ns.Arc(_u(r, 0.5, 0.7), _u(r, 0.1, 0.5), _u(r, 1.8, 2.8)))
leaf("sector", 2, "P_SECTOR")(lambda ns, r: ns.Sector(_u(r, 0.6, 0.9), _u(r, 0.1, 0.5), _u(r, 1.5, 2.2)))
leaf("infinite_sector", 2, "P_INFSECTOR")(lambda ns, r: ns.InfiniteSector(_u(r, 0.2, 0.6), _u(r, 1.3, 1.9)))
leaf("ngon_5", 2, "P_NGON")(lambda ns, r: ns.NGon(_u(r, 0.4, 0.7), 5))
leaf("ngon_17", 2, "P_NGON")(lambda ns, r: ns.NGon(_u(r, 0.4, 0.7), 17))       # beyond the rotation fold: by angle
leaf("segmented_line2", 2, "P_SEGLINE2")(lambda ns, r: ns.SegmentedLine(
    np.concatenate([r.uniform(-0.8, 0.8, (2, 5)), np.zeros((1, 5))])))
leaf("point_cloud2", 2, "P_NEAREST2")(lambda ns, r: ns.PointCloud2D(r.uniform(-0.8, 0.8, (3, 37))))
NEU_ORDERS = (1, 1.5, 2, 3, np.inf, -np.inf)          # kinds 0 (1 <= order), 1 (inf) and 2 (-inf)
for _order in NEU_ORDERS:
    leaf("neu_circle_%s" % str(_order).replace(".", "p").replace("-", "m"), 2, "P_NEUCIRCLE")(
        lambda ns, r, o=_order: ns.NEUCircle(_u(r, 0.4, 0.7), o))
del _order


# ---- C_C: coordinate maps ------------------------------------------------------------------------------------------------
def _box(ns, r):
    return ns.Box(_u(r, 0.4, 0.8), _u(r, 0.3, 0.6), _u(r, 0.2, 0.5))


def _elongate(b, r):
    """an ELONGATE between the placement and the map under test keeps Lowerer.emit from folding the two into one XFORM"""
    b.elongation((_u(r, 0.1, 0.3), _u(r, 0.0, 0.2), _u(r, 0.1, 0.3)))
    return b


@leaf("movc_displacement_in_union", 3, "MOVC VADD SYMMETRY VMIN")   # a register re-read after a child: the second field and
def _(ns, r):                                                   # the sibling see the untouched coordinates
    a = ns.Sphere(_u(r, 0.3, 0.45))
    a.symmetry(0)
    a.displacement(ns.sdf_x, (_u(r, -0.1, 0.1),))
    b = _box(ns, r)
    b.move((0.3, 0.1, 0.0))
    return ns.CombineGeometry("UNION2").combine(a, b)


@leaf("alias_symmetry_in_child", 3, "SYMMETRY VADD VMIN")             # the existing alias_symmetry_in_child_not_visible
def _(ns, r):
    a = ns.Sphere(_u(r, 0.25, 0.4))
    a.symmetry(0)
    b = _box(ns, r)
    b.move((0.3, 0.1, 0.0))
    u = ns.CombineGeometry("UNION2").combine(a, b)
    u.displacement(ns.sdf_x, (0.0,))
    return u


def _lin3_leaf(name, angle, factor):
    @leaf(name, 3, "LIN3")
    def _(ns, r):
        b = _box(ns, r)
        c, s, t = np.cos(0.5), np.sin(0.5), np.tan(angle)
        rot, shear = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]), np.array([[1, 0, t], [0, 1, 0], [0, 0, 1.0]])
        m = factor * rot.dot(shear)
        b.rotate_sdf(m)                                # any 3 x 3 matrix is accepted: LIN3 of its transpose
        return _elongate(b, r)


_lin3_leaf("lin3_stretch", 1.0, 1.6)                    # 2-norm 3.4
_lin3_leaf("lin3_shrink", 0.3, 0.35)                    # 2-norm 0.41


@leaf("lin3_shear", 3, "LIN3")
def _(ns, r):
    b = _box(ns, r)
    b.shear_xz(_u(r, 0.6, 1.0))
    return _elongate(b, r)


def _xform_sheared(name, angle, k):
    @leaf(name, 3, "XFORM VSCALE")                     # shear and scale fold into the placement: one sheared XFORM
    def _(ns, r):
        b = _box(ns, r)
        b.scale_sdf(k)
        b.shear_yz(angle)
        return b


_xform_sheared("xform_sheared_stretch", -1.0, 0.4)      # CSCALE 2.5 inside: 2-norm well above 1
_xform_sheared("xform_sheared_shrink", 0.4, 2.5)


def _cscale_leaf(name, k):
    @leaf(name, 3, "CSCALE VSCALE")
    def _(ns, r):
        b = _box(ns, r)
        b.scale_sdf(k)
        return _elongate(b, r)


_cscale_leaf("cscale_grow", 1.7)
_cscale_leaf("cscale_shrink", 0.55)
_cscale_leaf("cscale_negative", -0.8)


@leaf("elongate", 3, "ELONGATE")
def _(ns, r):
    return _elongate(_box(ns, r), r)


@leaf("revolve", 3, "REVOLVE P_BOX2")
def _(ns, r):
    a = ns.Rectangle(_u(r, 0.2, 0.4), _u(r, 0.2, 0.5))
    a.revolution(_u(r, 0.4, 0.7))
    return a


@leaf("axis_revolution", 3, "ROT2D AXREV P_CIRCLE")
def _(ns, r):
    b = ns.Circle(_u(r, 0.15, 0.3))
    b.axis_revolution(_u(r, 0.4, 0.7), _u(r, 0.2, 1.2))
    return b


@leaf("extrude_circle", 3, "ZEROZ P_ZSLAB EXTRUDE P_CIRCLE")
def _(ns, r):
    c = ns.Circle(_u(r, 0.3, 0.6))
    c.extrusion(_u(r, 0.4, 1.0))
    return c


def _symmetry_leaf(axis):
    @leaf("symmetry_%s" % "xyz"[axis], 3, "SYMMETRY")
    def _(ns, r):
        seg = ns.Line((0.1, -0.3, 0.2), (0.6, 0.4, -0.1))
        seg.rounding(_u(r, 0.05, 0.15))
        seg.symmetry(axis)
        return seg


for _axis in range(3):
    _symmetry_leaf(_axis)
del _axis


@leaf("mirror", 3, "FOLDX XFORM")
def _(ns, r):
    s = ns.Sphere(_u(r, 0.2, 0.4))
    s.mirror(tuple(r.uniform(-0.5, 0.0, 3)), tuple(r.uniform(0.1, 0.5, 3)))
    return s


# ---- folds of Lowerer.emit: consecutive in-place affine maps ------------------------------------------------------------
_ROT = np.array([[np.cos(0.7), -np.sin(0.7), 0.0], [np.sin(0.7), np.cos(0.7), 0.0], [0.0, 0.0, 1.0]])


@leaf("fold2_contraction_first", 3, "XFORM", rigid="none")     # CSCALE 2 (the field shrinks), then XLATE, in place on C0
def _(ns, r):
    b = _box(ns, r)
    b.move_sdf((0.2, -0.1, 0.05))
    b.scale_sdf(0.5)
    return b


@leaf("fold2_contraction_last", 3, "XFORM", rigid="none")
def _(ns, r):
    b = _box(ns, r)
    b.scale_sdf(0.5)
    b.move_sdf((0.2, -0.1, 0.05))
    return b


@leaf("fold3_contraction_first", 3, "XFORM", rigid="none")
def _(ns, r):
    b = _box(ns, r)
    b.scale_sdf(1.8)
    b.rotate_sdf(_ROT)
    b.scale_sdf(0.4)
    return b


@leaf("fold3_contraction_last", 3, "XFORM", rigid="none")
def _(ns, r):
    b = _box(ns, r)
    b.scale_sdf(0.4)
    b.shear_xz(0.5)
    b.scale_sdf(1.8)
    return b


@leaf("fold3_placed", 3, "XFORM")                                # the same behind a placement: four maps into one
def _(ns, r):
    b = _box(ns, r)
    b.scale_sdf(0.6)
    b.move_sdf((0.1, 0.2, -0.1))
    b.scale_sdf(1.5)
    return b


# ---- V_V: value maps -----------------------------------------------------------------------------------------------------
def _value_leaf(name, targets, apply, base=None):
    @leaf(name, 3, targets)
    def _(ns, r):
        o = ns.Sphere(_u(r, 0.4, 0.6)) if base is None else base(ns, r)
        apply(o, r)
        return o


_value_leaf("vsubc", "VSUBC", lambda o, r: o.rounding(_u(r, 0.05, 0.15)), base=_box)
_value_leaf("vaffine_shrink", "VAFFINE", lambda o, r: o.rounding_cs(0.15, 1.0), base=_box)      # factor 0.7
_value_leaf("vaffine_grow", "VAFFINE", lambda o, r: o.rounding_cs(-0.2, 1.0), base=_box)        # factor 1.4
_value_leaf("vabs", "VABS", lambda o, r: o.boundary())
_value_leaf("vneg", "VNEG", lambda o, r: o.invert(), base=_box)
_value_leaf("vonion", "VONION", lambda o, r: o.onion(_u(r, 0.05, 0.15)))
_value_leaf("vconcentric", "VCONCENTRIC", lambda o, r: o.concentric(_u(r, 0.1, 0.3)))
_value_leaf("vrelu_steep", "VRELU", lambda o, r: o.relu(0.4))                                           # factor 2.5
_value_leaf("vrelu_flat", "VRELU", lambda o, r: o.relu(2.5))                                            # factor 0.4
_value_leaf("vlinfall_steep", "VLINFALL", lambda o, r: o.linear_falloff(1.5, 0.5))                      # factor 3
_value_leaf("vlinfall_flat", "VLINFALL", lambda o, r: o.linear_falloff(0.5, 2.0))                       # factor 0.25
_value_leaf("vlinfall_mixed", "VLINFALL", lambda o, r: o.linear_falloff(2.0, 3.0))                      # 2 / 3


# ---- V_VV: two-value operations on two placed spheres -------------------------------------------------------------------
def _two(ns, r):
    a, b = ns.Sphere(_u(r, 0.35, 0.5)), ns.Box(_u(r, 0.4, 0.6), _u(r, 0.3, 0.5), _u(r, 0.3, 0.5))
    a.move((-0.25, 0.1, 0.0))
    b.rotate(0.6, (1, 2, -1))
    b.move((0.3, -0.15, 0.2))
    return a, b


def _two_value_leaf(name, target, operation, width=None):
    @leaf(name, 3, target)
    def _(ns, r):
        return combine(ns, operation, width, *_two(ns, r))


_two_value_leaf("pair_vadd", "VADD", "SUM")
_two_value_leaf("pair_vdiff", "VDIFF", "DIFFERENCE")
for _code, (_operation, _width) in COMBINERS.items():
    _two_value_leaf("pair_" + _code.lower(), _code, _operation, _width)
del _code, _operation, _width

LEAVES_3D = tuple(n for n, l in LEAVES.items() if l.dim == 3)
LEAVES_2D = tuple(n for n, l in LEAVES.items() if l.dim == 2)


# ---- PAIRS ---------------------------------------------------------------------------------------------------------------
class Pair:
    """tree(ns) = outer(combine(A, B)). `leaf`: the name of the LEAVES entry among A and B (the other member is the plain
    sphere / circle), `leaf_first`: whether it is A. `kept(ns, which)`: the tree of operand `which` (0: A, 1: B) alone under
    the same outer modifications, what the combiner returns where the other operand is irrelevant: a second operand of
    a subtraction enters negated."""

    def __init__(self, name, leaf_name, leaf_first, code, outer=None, targets=()):
        self.name, self.leaf, self.leaf_first, self.code, self.outer = name, leaf_name, leaf_first, code, outer
        self.dim = LEAVES[leaf_name].dim
        self.operation, self.width = COMBINERS[code]
        self.targets = tuple(targets)                   # the opcodes this entry places ABOVE its site

    def partner(self, ns):
        r = _rng("partner of " + self.leaf)
        kind = "subtract" if self.code in SUBTRACTIONS else "compare"
        at = PARTNER_AT.get((self.leaf, kind), (PARTNER_SUBTRACTED if kind == "subtract" else PARTNER)[self.dim])
        c = np.asarray(at[:3], dtype=np.float64)
        if (self.leaf, kind) not in PARTNER_AT:
            c = c + r.uniform(-0.05, 0.05, 3) * (1.0, 1.0, self.dim == 3)
        radius = at[3] if len(at) > 3 else PARTNER_RADIUS
        o = ns.Sphere(radius) if self.dim == 3 else ns.Circle(radius)
        o.move(tuple(c))
        return o

    def placed_leaf(self, ns):
        return shift(LEAVES[self.leaf].build(ns), LEAF_SHIFT[self.dim])

    def members(self, ns):
        a, b = self.placed_leaf(ns), self.partner(ns)
        return (a, b) if self.leaf_first else (b, a)

    def _finish(self, ns, g):
        return g if self.outer is None else self.outer(ns, g)

    def tree(self, ns):
        return self._finish(ns, combine(ns, self.operation, self.width, *self.members(ns)))

    def kept(self, ns, which):
        g = self.members(ns)[which]
        if which == 1 and self.code in SUBTRACTIONS:
            g.invert()                                   # inside the member's own frame: -(s f) = s (-f), exactly
        return self._finish(ns, ns.CombineGeometry("UNION").combine(g))

    def site(self, ns, lower_geometry):
        """Index (into cull_sites) of the site of combine(A, B): the sites inside the leaf come before it."""
        return len(lower_geometry(LEAVES[self.leaf].build(ns)).cull_sites)


for _code in COMBINERS:
    for _name in LEAVES:
        for _first in (True, False):
            _key = "%s_%s_%s" % (_code.lower(), "a" if _first else "b", _name)
            PAIRS[_key] = Pair(_key, _name, _first, _code)
del _code, _name, _first, _key


def above(name, targets, outer, code="SMIN3", leaf_name="box"):
    key = "above_" + name
    assert key not in PAIRS, key
    PAIRS[key] = Pair(key, leaf_name, True, code, outer, targets.split())


def _mod(method, *args):
    def outer(ns, g):
        getattr(g, method)(*args)
        return g
    return outer


def _placed(*ops):
    def outer(ns, g):
        for method, args in ops:
            getattr(g, method)(*args)
        return g
    return outer


def _with(operation, width=None, second=True):
    def outer(ns, g):
        c = ns.Torus(0.5, 0.15)
        c.rotate(0.8, (1, 0.5, -0.3))
        c.move((-0.2, 0.3, -0.25))
        return combine(ns, operation, width, *((g, c) if second else (c, g)))
    return outer


def _displaced(ns, g):
    g.symmetry(1)
    g.displacement(ns.sdf_x, (0.05,))
    h = ns.Sphere(0.3)
    h.move((0.0, 0.0, 0.6))
    return ns.CombineGeometry("UNION2").combine(g, h)


# C_C above the site: the coordinate register the two operands start from carries the factor into K
above("xform", "XFORM VSCALE", _placed(("rotate", (0.9, SKEW_AXIS)), ("move", ((0.1, -0.2, 0.15),)), ("set_scale", (0.6,))))
above("xlate", "XLATE", _mod("move", (0.15, -0.1, 0.2)))
above("lin3", "LIN3 ELONGATE", _placed(("shear_xz", (0.8,)), ("elongation", ((0.2, 0.1, 0.0),))))
above("cscale", "CSCALE VSCALE ELONGATE", _placed(("scale_sdf", (0.6,)), ("elongation", ((0.2, 0.1, 0.0),))))
above("cscale_grow", "CSCALE VSCALE ELONGATE", _placed(("scale_sdf", (1.7,)), ("elongation", ((0.2, 0.1, 0.0),))))
above("elongate", "ELONGATE", _mod("elongation", (0.3, 0.1, 0.2)))
above("revolve", "REVOLVE", _mod("revolution", 0.5), leaf_name="rectangle")
above("axis_revolution", "ROT2D AXREV", _mod("axis_revolution", 0.5, 0.6), leaf_name="rectangle")
above("extrude", "ZEROZ EXTRUDE", _mod("extrusion", 0.7), leaf_name="rectangle")
above("symmetry", "SYMMETRY", _mod("symmetry", 0))
above("mirror", "FOLDX XFORM", _mod("mirror", (-0.4, 0.1, -0.1), (0.5, -0.2, 0.2)))
above("movc", "MOVC SYMMETRY VADD VMIN", _displaced)
# V_V above the site
above("vscale", "VSCALE", _mod("set_scale", 1.6))
above("vsubc", "VSUBC", _mod("rounding", 0.08))
above("vaffine", "VAFFINE CSCALE", _mod("rounding_cs", 0.15, 1.0))
above("vabs", "VABS", _mod("boundary"))
above("vneg", "VNEG", _mod("invert"))
above("vonion", "VONION", _mod("onion", 0.07))
above("vconcentric", "VCONCENTRIC", _mod("concentric", 0.2))
above("vrelu", "VRELU", _mod("relu", 0.4))
above("vlinfall", "VLINFALL", _mod("linear_falloff", 1.5, 0.5))
# V_VV above the site, the combined pair as the first and as the second operand
above("vadd", "VADD", _with("SUM"))
above("vdiff", "VDIFF", _with("DIFFERENCE", second=False))
for _code, (_operation, _width) in COMBINERS.items():
    above(_code.lower(), _code, _with(_operation, _width, second=_code in ("VMIN", "SMIN3", "VSUBTRACT", "SMAX3")),
          code="VMIN" if _code != "VMIN" else "SMIN3")
del _code, _operation, _width

# ten entries spread over the combiners, for the ray and occupancy tests
PAIRS_FOR_RAYS = ("vmin_a_lin3_stretch", "vmax_b_vrelu_steep", "vsubtract_a_cscale_shrink", "smin2_b_vlinfall_steep",
                  "smin3_a_xform_sheared_stretch", "smax3_a_box_grown", "ssub3_b_vaffine_grow", "smin3_b_pair_vadd",
                  "vmin_b_fold3_contraction_first", "above_lin3")
PAIRS_FOR_OCCUPANCY_2D = ("vmin_a_neu_circle_1p5", "smin3_b_rounded_rectangle", "vsubtract_a_ngon_17")


# ---- CHAINS --------------------------------------------------------------------------------------------------------------
CHAIN_MEMBERS = 24            # above the default SDFK_CHAIN_MIN of 22: table-driven chain mode, any SDFK_CHAIN_KMAX


def chain_pool(dim):
    """The leaves a chain cycles through: a member with a combiner of its own (a cull site inside an operand) keeps the
    combination out of chain mode (csrc/sdfk_codegen.cpp chain_analyse); those leaves are covered by PAIRS."""
    return tuple(n for n, l in LEAVES.items() if l.dim == dim and not (set(l.targets) & (set(COMBINERS) | {"MOVC"})))


class Chain:
    def __init__(self, name, operation, dim, first):
        self.name, self.operation, self.dim, self.first = name, operation, dim, first

    def member_names(self):
        pool = chain_pool(self.dim)
        return [pool[(self.first + i) % len(pool)] for i in range(CHAIN_MEMBERS)]

    def members(self, ns):
        r = _rng(self.name)
        members = []
        for n in self.member_names():
            t = r.uniform(-0.6, 0.6, 3)
            members.append(shift(LEAVES[n].build(ns), (t[0], t[1], t[2] if self.dim == 3 else 0.0)))
        return members

    def tree(self, ns):
        return ns.CombineGeometry(self.operation).combine(*self.members(ns))


for _dim in (3, 2):
    _count = len(chain_pool(_dim))
    for _k in range((_count + CHAIN_MEMBERS - 1) // CHAIN_MEMBERS):           # every leaf is a member of some chain
        for _operation in ("UNION", "INTERSECT"):
            _key = "%s_%dd_%d" % (_operation.lower(), _dim, _k)
            CHAINS[_key] = Chain(_key, _operation, _dim, _k * CHAIN_MEMBERS)
del _dim, _count, _k, _operation, _key


# ---- UNBOUNDED -----------------------------------------------------------------------------------------------------------
def unbounded(name, dim=3):
    def deco(fn):
        UNBOUNDED[name] = (fn, dim)
        return fn
    return deco


@unbounded("twist")
def _(ns):
    b = ns.Box(0.6, 0.3, 0.5)
    b.twist(0.8)
    return b


@unbounded("bend")
def _(ns):
    b = ns.Box(1.6, 0.3, 0.25)
    b.bend(1.5, np.pi / 3)
    return b


@unbounded("infinite_repetition")
def _(ns):
    a = ns.Sphere(0.3)
    a.infinite_repetition((1.1, 1.3, 1.7))
    return a


@unbounded("finite_repetition")
def _(ns):
    a = ns.Box(0.3, 0.2, 0.25)
    a.finite_repetition((1.5, 1.2, 1.6), (3, 3, 4))
    return a


@unbounded("sign")
def _(ns):
    a = ns.Sphere(0.5)
    a.sign()
    return a


@unbounded("quad_bent")                       # four vertices that are not coplanar: the field jumps (see DESIGN)
def _(ns):
    return ns.Quad((-0.6, -0.5, 0.0), (0.6, -0.6, 0.3), (0.7, 0.5, 0.0), (-0.5, 0.6, 0.0))


NEU_UNBOUNDED_ORDERS = (0.3, 0.5, 0.75, 0.99, 0)          # order < 1: unbounded slope at the axes; order 0: kind 3
for _order in NEU_UNBOUNDED_ORDERS:
    unbounded("neu_circle_%s" % str(_order).replace(".", "p"), 2)(lambda ns, o=_order: ns.NEUCircle(0.6, o))
del _order


def union_with_circle(ns, member):
    """The regression geometry of the NEUCircle finding: UNION(member, Circle(0.3))."""
    return ns.CombineGeometry("UNION").combine(member, ns.Circle(0.3))


def grid(dim):
    """-> (float64 axes, (3, n) float64 points in the order of generate_grid: the last axis runs fastest; 2-D: z = 0)."""
    shape, extents = GRID_3D if dim == 3 else GRID_2D
    axes = [np.linspace(lo, hi, m).astype(np.float32).astype(np.float64) for m, (lo, hi) in zip(shape, extents)]
    co = np.zeros((3, int(np.prod(shape))))
    co[:dim] = np.asarray(np.meshgrid(*axes, indexing="ij")).reshape(dim, -1)
    return axes, co
