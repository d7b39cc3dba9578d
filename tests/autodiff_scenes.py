"""Geometries for the forward-mode derivative tests (aegolius_amd.autodiff).

Every entry of SCENES is `name -> (builder(ns), primals, argnums)`: `builder(ns)` returns the builder — a callable that
takes the primals and returns a geometry of namespace `ns` — so that the same text drives aegolius_amd.cores and the
oracle (which evaluates the same objects in float64). Citations "E/" are to examples/autodiff/ of the reference.
"""
import numpy as np

SCENES = {}


def scene(name, primals, argnums):
    def deco(fn):
        assert name not in SCENES, name
        SCENES[name] = (fn, tuple(primals), argnums)
        return fn
    return deco


# ---- the reference's autodiff scripts, restated with the object API ----------------------------------------------------
@scene("gradient_map_parameters", (1.0,), 0)          # E/gradient_map_parameters.py:34-38: sdf_circle, d/d radius
def _(ns):
    return lambda r: ns.Circle(r)


@scene("gradient_map_transformations", (0.0, 0.0, 1.0), (0, 1, 2))   # E/gradient_map_transformations.py:50-60
def _(ns):
    def build(x0, y0, r):
        c = ns.Circle(r)
        c.move((x0, y0, 0))
        return c
    return build


@scene("gradient_map_modifications", (1.0, 2.0, 0.2), (0, 1, 2))     # E/gradient_map_modifications.py:50-60
def _(ns):
    def build(r, d, w):
        c = ns.Circle(r)
        c.onion(w)
        c.mirror((-d / 2, 0, 0), (d / 2, 0, 0))
        c.rotate(np.pi / 4, (0, 0, 1))
        return c
    return build


@scene("gradient_map_combine", (1.0, 1.0, 0.2, 0.2), (0, 1, 2, 3))   # E/gradient_map_combine.py:55-75
def _(ns):
    def build(r, d, w, s):
        a, b = ns.Circle(r), ns.Circle(r)
        a.move((-d / 2, 0, 0))
        b.move((d / 2, 0, 0))
        u = ns.CombineGeometry("SMOOTH_UNION2").combine_parametric(a, b, parameters=s)
        u.onion(w)
        u.rotate(np.pi / 4, (0, 0, 1))
        return u
    return build


@scene("gradient_map_3D", (2.0, 30.0, 0.5, 1.8), (0, 1, 2, 3))       # E/gradient_map_3D.py:55-72
def _(ns):
    def arc(r, w, a_deg, z):
        o = ns.Arc3D(r, 0.0, np.pi * 5 / 6, -np.pi * 5 / 6)
        o.concentric(w)
        o.elongation((0.0, 0.0, 0.75 / 2))
        if a_deg is not None:
            o.rotate(np.deg2rad(a_deg), (0, 0, 1))
            o.move((0, 0, z))
            o.set_scale(1.2)
        return o

    def build(r, a, w, s):
        u = ns.CombineGeometry("UNION2").combine(arc(r, w, a, 1.5), arc(r, w, -a, -1.5))
        u = ns.CombineGeometry("SMOOTH_UNION2").combine_parametric(u, arc(r, w, None, 0), parameters=s)
        u.onion(0.1)
        return u
    return build


@scene("position_optimization", (0.3, -0.2), (0, 1))                # E/position_optimization.py:62-86
def _(ns):
    def build(x0, y0):
        c = ns.Circle(1.0)
        c.gaussian_falloff(1.0, 0.5)
        c.move((x0, y0, 0))
        return c
    return build


@scene("multi_position_optimization", (np.array([0.0, 0.1, -1.0]), np.array([0.0, 0.2, 0.5])), (0, 1))
def _(ns):                                              # E/multi_position_optimization.py:68-110 (pure SDF, hard union)
    def build(xs, ys):
        cs = []
        for x, y in zip(xs, ys):
            c = ns.Circle(1.0)
            c.move((x, y, 0))
            cs.append(c)
        return ns.CombineGeometry("UNION").combine(*cs)
    return build


AUTODIFF_SCRIPTS = tuple(SCENES)


# ---- one parametrised builder per covered op family ----------------------------------------------------------------
def _placed(o, angle, move):
    o.rotate(angle, (0.3, -0.5, 0.8))
    o.move(move)
    return o


@scene("fam_sphere_box_cyl", (0.4, 0.5, 0.3, 0.25), (0, 1, 2, 3))
def _(ns):
    def build(r, a, h, ang):
        u = ns.CombineGeometry("UNION").combine(
            _placed(ns.Sphere(r), ang, (0.3, 0.1, 0.0)), _placed(ns.Box(a, 0.4, 0.3), 0.3, (-0.4, 0.2, 0.1)),
            _placed(ns.Cylinder(0.2, h), 0.5, (0.1, -0.5, 0.2)))
        return u
    return build


@scene("fam_torus_chainlink_cone", (0.3, 0.1, 0.6), (0, 1, 2))
def _(ns):
    def build(R, r, hgt):
        t = _placed(ns.Torus(R, r), 0.4, (0.2, 0.0, 0.1))
        c = _placed(ns.ChainLink(R, r, 0.3), 0.9, (-0.3, 0.2, 0.0))
        k = _placed(ns.Cone(hgt, np.pi / 8), 0.2, (0.0, -0.2, -0.3))
        return ns.CombineGeometry("SMOOTH_INTERSECT2").combine_parametric(
            ns.CombineGeometry("UNION2").combine(t, c), k, parameters=0.3)
    return build


@scene("fam_2d_prims", (0.4, 0.8, 0.35, 0.1), (0, 1, 2, 3))
def _(ns):
    def build(r, a, ng, rr):
        c = _placed(ns.Circle(r), 0.0, (0.2, 0.1, 0.0))
        b = ns.Rectangle(a, 0.5)
        b.move((-0.3, 0.2, 0))
        g = ns.NGon(ng, 5)
        g.move((0.1, -0.3, 0))
        q = ns.RoundedRectangle(0.8, 0.6, (rr, 0.05, 0.15, 0.0))
        q.move((0.3, 0.3, 0))
        t = ns.Triangle((-0.5, -0.4, 0), (0.3, -0.3, 0), (0.0, 0.4, 0))
        return ns.CombineGeometry("SMOOTH_UNION2").combine_parametric(
            ns.CombineGeometry("UNION").combine(c, b, g), ns.CombineGeometry("UNION2").combine(q, t), parameters=0.1)
    return build


@scene("fam_mods", (0.2, 0.5, 0.3), (0, 1, 2))
def _(ns):
    def build(e, pitch, ang):
        b = ns.Box(0.6, 0.3, 0.2)
        b.elongation((e, 0, 0.1))
        b.twist(pitch)
        b.bend(1.5, np.pi / 3)
        b.rotate(ang, (0, 1, 1))
        b.move((0.1, -0.2, 0.05))
        return b
    return build


@scene("fam_value_mods", (0.05, 0.3, 0.2), (0, 1, 2))
def _(ns):
    def build(w, s, k):
        a = ns.Sphere(0.5)
        a.rounding(w)
        a.scale_sdf(1.0 + k)
        b = ns.Box(0.6, 0.5, 0.4)
        b.onion(w)
        b.move((0.3, 0, 0))
        u = ns.CombineGeometry("SMOOTH_SUBTRACT2").combine_parametric(a, b, parameters=s)
        u.sigmoid_falloff(1.0, 0.4)
        return u
    return build


@scene("fam_symmetry_rotsym", (0.25, 0.5, 0.4), (0, 1, 2))
def _(ns):
    def build(r, phase, rad):
        s = ns.Sphere(r)
        s.move((0.3, 0.2, 0.1))
        s.symmetry(0)
        s.rotational_symmetry(5, rad, phase)
        return s
    return build


@scene("fam_boltz_extrude", (0.3, 0.4, 0.5), (0, 1, 2))
def _(ns):
    def build(w, r, d):
        c = ns.Circle(r)
        c.extrusion(d)
        b = ns.Box(0.4, 0.6, 0.3)
        b.move((0.3, 0.1, 0))
        return ns.CombineGeometry("SMOOTH_INTERSECT2_BOLTZMANN").combine_parametric(c, b, parameters=w)
    return build


@scene("cfg2_width", (0.1,), 0)                          # BASELINE cfg 2 with the smoothing width as the parameter
def _(ns):
    from aegolius_amd import workloads
    return lambda w: workloads.cfg2_tree(ns, width=w)


@scene("fam_repetitions", (0.3, 1.1, 0.9), (0, 1, 2))
def _(ns):
    def build(r, d, b):
        a = ns.Sphere(r)
        a.infinite_repetition((d, 1.3, 1.7))
        f = ns.Box(r, 0.2, 0.3)
        f.finite_repetition((2.0 * d, 1.5, 1.5), (3, 2, 2))
        g = ns.Sphere(0.15)
        g.linear_instancing(4, (-b, -0.3, 0.1), (b, 0.4, -0.2))
        return ns.CombineGeometry("UNION").combine(a, f, g)
    return build


@scene("fam_revolutions", (0.6, 0.4, 0.3), (0, 1, 2))
def _(ns):
    def build(R, ang, h):
        a = ns.Rectangle(0.3, h)
        a.revolution(R)
        b = ns.Circle(0.2)
        b.axis_revolution(R, ang)
        b.move((0.2, 0.1, 0.3))
        return ns.CombineGeometry("UNION2").combine(a, b)
    return build


@scene("fam_linear_maps", (0.3, 0.5, 0.2), (0, 1, 2))
def _(ns):
    def build(t, ang, x0):
        b = ns.Box(0.6, 0.4, 0.5)
        b.shear_xz(t)
        c, s = np.cos(ang), np.sin(ang)
        b.rotate_sdf(np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]))
        b.move_sdf((x0, -0.1, 0.05))
        return b
    return build


@scene("fam_axes_planes_segments", (0.2, 0.4, 0.3, 0.5), (0, 1, 2, 3))
def _(ns):
    def build(o, ang, th, bx):
        x = ns.X(o)
        p = ns.OrientedPlane((np.cos(ang), np.sin(ang), 0.0), 0.1)
        slab = ns.Plane((0.0, 0.3, 1.0), th)
        seg = ns.Line((-0.4, 0.2, -0.1), (bx, -0.3, 0.4))
        seg.rounding(0.1)
        y, z = ns.Y(-0.2), ns.Z(0.3)
        inter = ns.CombineGeometry("INTERSECT").combine(x, p, y, z)
        return ns.CombineGeometry("SUBTRACT2").combine(ns.CombineGeometry("UNION2").combine(inter, seg), slab)
    return build


@scene("fam_2d_arc_segment", (0.6, 2.0, 0.3, 0.2), (0, 1, 2, 3))
def _(ns):
    def build(r, a2, by, w):
        arc = ns.Arc(r, 0.3, a2)
        arc.onion(0.05)
        seg = ns.Segment((-0.5, -0.2, 0.0), (0.4, by, 0.0))
        seg.onion(0.04)
        box = ns.Rectangle(0.5, 0.4)
        box.move((0.2, -0.3, 0))
        u = ns.CombineGeometry("SMOOTH_UNION2_2").combine_parametric(arc, seg, parameters=w)
        return ns.CombineGeometry("SMOOTH_SUBTRACT2_BOLTZMANN").combine_parametric(u, box, parameters=w)
    return build


@scene("fam_value_ops", (0.1, 0.4, 0.25), (0, 1, 2))
def _(ns):
    def build(rr, k, r):
        a = ns.Box(0.8, 0.6, 0.5)
        a.rounding_cs(rr, 1.0)
        b = ns.Sphere(r)
        b.boundary()
        b.invert()
        c = ns.Sphere(0.5)
        c.move((0.2, 0.1, 0.0))
        d = ns.Box(0.4, 0.4, 0.4)
        d.scale_sdf(1.0 + k)
        s = ns.CombineGeometry("SUM").combine(a, b)
        t = ns.CombineGeometry("DIFFERENCE").combine(c, d)
        e = ns.Sphere(0.6)
        e.recover_volume(ns.Box(0.9, 0.9, 0.9 + k).propagate)
        return ns.CombineGeometry("UNION").combine(s, t, e)
    return build


@scene("fam_value_maps", (0.5, 0.6, 0.7, 0.8, 0.4, 0.3, 0.5, 0.1), (0, 1, 2, 3, 4, 5, 6, 7))
def _(ns):
    """every post-processing map with its own parameter as the primal (eight channels: two launches)"""
    def build(w1, w2, w3, w4, w5, w6, w7, thr):
        objs = []
        for i, apply in enumerate((lambda o: o.sigmoid_falloff(1.0, w1), lambda o: o.positive_sigmoid_falloff(w2, 0.5),
                                   lambda o: o.capped_exponential(1.0, w3), lambda o: o.linear_falloff(w4, 0.9),
                                   lambda o: o.relu(w5), lambda o: o.smooth_relu(w6, 1.0, 0.05),
                                   lambda o: o.slowstart(0.3, w7, 0.05, True), lambda o: o.gaussian_boundary(1.0, w1),
                                   lambda o: o.hard_binarization(thr), lambda o: o.sign())):
            o = ns.Sphere(0.3 + 0.05 * i)
            o.move((0.1 * i - 0.4, 0.05 * i, -0.1))
            apply(o)
            objs.append(o)
        return ns.CombineGeometry("UNION").combine(*objs)
    return build


# ---- point mode (value_and_grad_points): the default lowering, with the ops only it emits ---------------------------
POINT_SCENES = {}


def point_scene(name):
    def deco(fn):
        POINT_SCENES[name] = fn
        return fn
    return deco


@point_scene("recover_volume_in_union")         # an identity-framed operand re-read by its second field: MOVC
def _(ns):
    a = ns.Sphere(0.6)
    a.recover_volume(ns.Box(0.8, 0.7, 0.9).propagate)
    b = ns.Box(0.3, 0.4, 0.5)
    b.move((0.4, 0.2, 0.1))
    return ns.CombineGeometry("UNION").combine(a, b)


@point_scene("sign_of_gaussian")                # sign() of a positive map: VEXPFLAG
def _(ns):
    a = ns.Sphere(0.5)
    a.gaussian_falloff(1.0, 0.5)
    a.sign()
    b = ns.Torus(0.5, 0.2)
    b.rotate(0.4, (1, 0, 0))
    return ns.CombineGeometry("SUM").combine(a, b)


@point_scene("cfg3_mod_chain")
def _(ns):
    from aegolius_amd import workloads
    return workloads.cfg3_chain(ns)


# ---- parameter tangents the scenes above leave at zero ----------------------------------------------------------------
@scene("fam_bend_parameters", (1.5, 1.0), (0, 1))       # both branches of BEND with all six parameters moving
def _(ns):
    def build(R, a):
        b = ns.Box(1.6, 0.3, 0.25)
        b.bend(R, a)
        b.rotate(0.3, (0.3, -0.5, 0.8))
        b.move((0.1, -0.2, 0.05))
        return b
    return build


@scene("fam_triangle_smax_parameters", (-0.5, 0.4, 0.3), (0, 1, 2))   # a triangle vertex and the width of SMAX3
def _(ns):
    def build(ax, cy, w):
        t = ns.Triangle((ax, -0.4, 0), (0.5, -0.3, 0), (0.0, cy, 0))
        c = ns.Circle(0.6)
        c.move((0.2, 0.1, 0))
        return ns.CombineGeometry("SMOOTH_INTERSECT2").combine_parametric(t, c, parameters=w)
    return build


# ---- one geometry per dual rule, behind an explicit skew placement ------------------------------------------------------
# OP_GEOMETRIES: name -> (make(ns, tx, ty, ang, s), dim, targets, regions). `make` builds the geometry with constant
# arguments, applies every modification, and places the result LAST with rotate(ang, axis), move((tx, ty, z0)),
# set_scale(s): the coordinate that reaches the modification and the primitive then has live tangents in all its
# components, in point mode (∇_x) and in parameter mode (d/d tx, ty, ang, s). `targets` are the opcodes the entry exists
# for. `regions(local)`, where the rule branches, labels every point with the branch it takes: `local` are the float64
# coordinates behind the placement (local_coordinates below); a predicate that needs the coordinate behind an earlier
# modification (the frame of mirror / linear_instancing, the ROT2D of rotational_symmetry) applies it itself.
# `regions.labels` names the labels: a tuple of names for an (n,) result, a tuple of such tuples for a (k, n) result
# (k independent branch points, e.g. one per axis).
OP_GEOMETRIES = {}
OP_DEFAULTS = (0.2, -0.1, 0.4, 1.2)
OP_IDENTITY = (0.0, 0.0, 0.0, 1.0)
SKEW_AXIS = (0.3, -0.5, 0.8)
PLACE_Z = 0.15                      # the constant z of a 3-D entry's move


def place(o, dim, tx, ty, ang, s):
    o.rotate(ang, SKEW_AXIS if dim == 3 else (0, 0, 1))
    o.move((tx, ty, PLACE_Z if dim == 3 else 0.0))
    o.set_scale(s)
    return o


def local_coordinates(geo, co):
    """The coordinates the placed expression is evaluated at: R^T co / s - R^T t (reference transformations.py:232-242)."""
    R = np.asarray(geo.rotation_matrix, dtype=np.float64)
    t = np.asarray(geo.center, dtype=np.float64).reshape(3)
    return R.T.dot(np.asarray(co, dtype=np.float64)) / float(geo.scale) - R.T.dot(t)[:, None]


def labelled(*labels):
    def deco(fn):
        fn.labels = labels
        return fn
    return deco


def op_geometry(name, dim, targets, regions=None):
    def deco(fn):
        assert name not in OP_GEOMETRIES, name

        def make(ns, tx, ty, ang, s):
            return place(fn(ns), dim, tx, ty, ang, s)
        OP_GEOMETRIES[name] = (make, dim, tuple(targets.split()), regions)
        return fn
    return deco


def _count_positive(*q):
    return sum((x > 0).astype(np.int64) for x in q)


# -- coordinate plumbing --
@op_geometry("movc_recover_volume", 3, "MOVC VMUL")      # default lowering: the operand re-read by its second field
def _(ns):
    a = ns.Sphere(0.6)
    a.recover_volume(ns.Box(0.8, 0.7, 0.9).propagate)
    b = ns.Box(0.3, 0.4, 0.5)
    b.move((0.4, 0.2, 0.1))
    return ns.CombineGeometry("UNION").combine(a, b)


@op_geometry("xform_nested", 3, "XFORM VSCALE VMIN")     # a placed child inside the placed union
def _(ns):
    a = ns.Box(0.5, 0.4, 0.3)
    a.rotate(0.7, (1, 2, -1))
    a.move((-0.3, 0.2, 0.1))
    b = ns.Sphere(0.3)
    b.move((0.35, -0.1, 0.2))
    b.set_scale(1.3)
    return ns.CombineGeometry("UNION2").combine(a, b)


@op_geometry("xlate_moved_children", 3, "XLATE")         # default lowering: a child that is only moved
def _(ns):
    a = ns.Box(0.5, 0.4, 0.3)
    a.move((-0.3, 0.2, 0.1))
    b = ns.Torus(0.3, 0.1)
    b.move((0.35, -0.1, 0.2))
    return ns.CombineGeometry("SMOOTH_UNION2").combine_parametric(a, b, parameters=0.2)


@op_geometry("xlate_move_sdf", 3, "XLATE TWIST")         # move_sdf behind a twist: XLATE in both lowerings
def _(ns):
    b = ns.Box(0.6, 0.4, 0.5)
    b.move_sdf((0.2, -0.1, 0.05))
    b.twist(0.5)
    return b


@op_geometry("lin3_shear", 3, "LIN3")                    # behind an elongation, or the default lowering folds it away
def _(ns):
    b = ns.Box(0.6, 0.4, 0.5)
    b.shear_xz(0.3)
    b.elongation((0.2, 0.1, 0.15))
    return b


@op_geometry("lin3_rotate_sdf", 3, "LIN3")
def _(ns):
    b = ns.Box(0.6, 0.4, 0.5)
    c, s = np.cos(0.5), np.sin(0.5)
    b.rotate_sdf(np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]))
    b.twist(0.4)
    return b


@op_geometry("cscale_scale_sdf", 3, "CSCALE VSCALE")
def _(ns):
    b = ns.Box(0.6, 0.4, 0.5)
    b.scale_sdf(1.3)
    b.elongation((0.2, 0.1, 0.15))
    return b


@labelled(("x inside", "x outside"), ("y inside", "y outside"), ("z inside", "z outside"))
def _elongate_regions(l):
    e = np.array([[0.45], [0.4], [0.45]])
    return (np.abs(l) > e).astype(np.int64)


@op_geometry("elongate_box", 3, "ELONGATE", _elongate_regions)
def _(ns):
    b = ns.Box(0.5, 0.4, 0.3)
    b.elongation((0.9, 0.8, 0.9))
    return b


@op_geometry("revolve_rectangle", 3, "REVOLVE P_BOX2")
def _(ns):
    a = ns.Rectangle(0.3, 0.4)
    a.revolution(0.6)
    return a


@op_geometry("axis_revolution_circle", 3, "ROT2D AXREV P_CIRCLE")
def _(ns):
    b = ns.Circle(0.2)
    b.axis_revolution(0.6, 0.4)
    return b


@labelled("inside", "side", "cap", "edge")
def _extrude_regions(l):
    a, b = np.hypot(l[0], l[1]) - 0.6, np.abs(l[2]) - 0.5
    return (a > 0).astype(np.int64) + 2 * (b > 0)


@op_geometry("extrude_circle", 3, "ZEROZ P_ZSLAB EXTRUDE", _extrude_regions)
def _(ns):
    c = ns.Circle(0.6)
    c.extrusion(1.0)
    return c


@op_geometry("extrude_ngon", 3, "ZEROZ P_ZSLAB EXTRUDE P_NGON")
def _(ns):
    g = ns.NGon(0.5, 5)
    g.extrusion(0.8)
    return g


@op_geometry("twist_box", 3, "TWIST")
def _(ns):
    b = ns.Box(0.6, 0.3, 0.5)
    b.twist(0.8)
    return b


@labelled("arc", "straight x >= 0", "straight x < 0")
def _bend_regions(l):
    R, a = 1.5, np.pi / 3
    phi = np.arctan2(l[0], R - l[1])
    straight = R * a / 2 <= np.abs(R * phi)
    return np.where(straight, np.where(l[0] >= 0, 1, 2), 0)


@op_geometry("bend_box", 3, "BEND", _bend_regions)
def _(ns):
    b = ns.Box(1.6, 0.3, 0.25)
    b.bend(1.5, np.pi / 3)
    return b


@op_geometry("infrep_sphere", 3, "INFREP")
def _(ns):
    a = ns.Sphere(0.3)
    a.infinite_repetition((1.1, 1.3, 1.7))
    return a


_FINREP = (np.array([1.5, 1.2, 1.6]), np.array([3.0, 3.0, 4.0]))


@labelled(("x span", "x above", "x below"), ("y span", "y above", "y below"), ("z span", "z above", "z below"))
def _finrep_regions(l):
    size, rep = _FINREP
    d = (size * (0.5 - 1.0 / rep))[:, None]
    return np.where(l > d, 1, np.where(l < -d, 2, 0))


@op_geometry("finrep_box", 3, "FINREP", _finrep_regions)
def _(ns):
    f = ns.Box(0.3, 0.2, 0.25)
    f.finite_repetition(tuple(_FINREP[0]), tuple(int(r) for r in _FINREP[1]))
    return f


def _off_centre_rod(ns):
    seg = ns.Line((0.1, -0.3, 0.2), (0.6, 0.4, -0.1))
    seg.rounding(0.1)
    return seg


def _symmetry_entry(axis):
    @labelled("positive", "negative")
    def regions(l):
        return (l[axis] < 0).astype(np.int64)

    @op_geometry("symmetry_%s" % "xyz"[axis], 3, "SYMMETRY", regions)
    def _(ns):
        seg = _off_centre_rod(ns)
        seg.symmetry(axis)
        return seg


for _axis_ in range(3):
    _symmetry_entry(_axis_)
del _axis_


def _frame_x(l, a, b):
    """x of the frame of mirror / linear_instancing (reference modifications.py:978-988): along b - a, from the middle."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    w = b - a
    return (w / np.linalg.norm(w)).dot(l - ((a + b) / 2)[:, None])


_MIRROR = ((-0.3, 0.1, -0.1), (0.4, -0.2, 0.2))


@labelled("positive", "negative")
def _foldx_regions(l):
    return (_frame_x(l, *_MIRROR) < 0).astype(np.int64)


@op_geometry("mirror_sphere", 3, "FOLDX", _foldx_regions)
def _(ns):
    s = ns.Sphere(0.3)
    s.mirror(*_MIRROR)
    return s


@labelled("sector 0", "sector 1", "sector 2")
def _rotsym_regions(l):
    angle, phase = 2 * np.pi / 3, 0.5
    h = angle / 2 - phase
    x, y = np.cos(h) * l[0] + np.sin(h) * l[1], -np.sin(h) * l[0] + np.cos(h) * l[1]
    return np.minimum(np.floor(np.mod(np.arctan2(y, x), 2 * np.pi) / angle), 2).astype(np.int64)


@op_geometry("rotsym_rod", 3, "ROT2D ROTSYM", _rotsym_regions)
def _(ns):
    seg = _off_centre_rod(ns)
    seg.rotational_symmetry(3, 0.4, 0.5)
    return seg


_LININST = (4, (-0.8, -0.3, 0.1), (0.7, 0.4, -0.2))


@labelled("span", "above", "below")
def _lininst_regions(l):
    n, a, b = _LININST
    x = _frame_x(l, a, b)
    length = np.linalg.norm(np.subtract(b, a))
    hi = length / 2 - length / (n - 1) / 2
    return np.where(x > hi, 1, np.where(x < -hi, 2, 0))


@op_geometry("lininst_sphere", 3, "LININST", _lininst_regions)
def _(ns):
    g = ns.Sphere(0.15)
    g.linear_instancing(*_LININST)
    return g


# -- 3-D primitives --
@op_geometry("axes_xyz", 3, "P_AXIS VMAX")
def _(ns):
    return ns.CombineGeometry("INTERSECT").combine(ns.X(0.2), ns.Y(-0.2), ns.Z(0.3))


@op_geometry("sphere", 3, "P_SPHERE VSCALE")
def _(ns):
    return ns.Sphere(0.5)


@labelled("inside", "side", "cap", "edge")
def _cylinder_regions(l):
    return (np.hypot(l[0], l[1]) - 0.6 > 0).astype(np.int64) + 2 * (np.abs(l[2]) - 0.5 > 0)


@op_geometry("cylinder", 3, "P_CYLINDER", _cylinder_regions)
def _(ns):
    return ns.Cylinder(0.6, 1.0)


@labelled("inside", "face", "edge", "corner")
def _box_regions(l):
    return _count_positive(np.abs(l[0]) - 0.6, np.abs(l[1]) - 0.5, np.abs(l[2]) - 0.45)


@op_geometry("box", 3, "P_BOX", _box_regions)
def _(ns):
    return ns.Box(1.2, 1.0, 0.9)


@op_geometry("torus", 3, "P_TORUS")
def _(ns):
    return ns.Torus(0.5, 0.15)


@op_geometry("chainlink", 3, "P_CHAINLINK")
def _(ns):
    return ns.ChainLink(0.3, 0.1, 0.6)


def _arc_regions(a0, a1):
    @labelled("body", "end cap")
    def regions(l):
        mid, hw = (a0 + a1) / 2, abs(a1 - (a0 + a1) / 2)
        x, y = np.cos(mid) * l[0] + np.sin(mid) * l[1], np.abs(-np.sin(mid) * l[0] + np.cos(mid) * l[1])
        return (np.arctan2(y, x) >= hw).astype(np.int64)
    return regions


@op_geometry("arc3d", 3, "P_ARC3D", _arc_regions(0.3, 2.6))
def _(ns):
    return ns.Arc3D(0.6, 0.1, 0.3, 2.6)


@op_geometry("oriented_plane", 3, "P_PLANE")
def _(ns):
    return ns.OrientedPlane((0.6, 0.0, 0.8), 0.1)


@op_geometry("plane_slab", 3, "P_UPLANE")
def _(ns):
    return ns.Plane((0.0, 0.6, 0.8), 0.3)


def _segment_regions(a, b):
    @labelled("interior", "end a", "end b")
    def regions(l):
        a_, ba = np.asarray(a, dtype=np.float64), np.subtract(b, a).astype(np.float64)
        t = ba.dot(l[:a_.size] - a_[:, None]) / ba.dot(ba)
        return np.where(t < 0, 1, np.where(t > 1, 2, 0))
    return regions


_SEG3 = ((-0.4, 0.2, -0.3), (0.5, -0.3, 0.4))


@op_geometry("segment3", 3, "P_SEGMENT3", _segment_regions(*_SEG3))
def _(ns):
    return ns.Line(*_SEG3)


_CONE = (0.6, np.pi / 5)


@labelled("side", "apex", "rim", "base")
def _cone_regions(l):
    """The branches of dual_prim_cone: the nearer of the side segment (clipped at the apex / the rim) and the base."""
    h, ang = _CONE
    q0, q1 = h * np.tan(ang), -h
    w0, w1 = np.hypot(l[0], l[1]), l[2] - h * 0.5 ** (1.0 / 3.0)
    u1 = (w0 * q0 + w1 * q1) / (q0 * q0 + q1 * q1)
    t1 = np.clip(u1, 0, 1)
    u2 = w0 / q0
    t2 = np.clip(u2, 0, 1)
    da = (w0 - q0 * t1) ** 2 + (w1 - q1 * t1) ** 2
    db = (w0 - q0 * t2) ** 2 + (w1 - q1) ** 2
    side = da <= db
    rim = (side & (u1 >= 1)) | (~side & (u2 >= 1))
    return np.where(rim, 2, np.where(side, np.where(u1 <= 0, 1, 0), 3))


@op_geometry("cone", 3, "P_CONE", _cone_regions)
def _(ns):
    return ns.Cone(*_CONE)


# -- 2-D primitives --
@op_geometry("circle", 2, "P_CIRCLE")
def _(ns):
    return ns.Circle(0.5)


@labelled("inside", "face", "corner")
def _box2_regions(l):
    return _count_positive(np.abs(l[0]) - 0.5, np.abs(l[1]) - 0.35)


@op_geometry("rectangle", 2, "P_BOX2", _box2_regions)
def _(ns):
    return ns.Rectangle(1.0, 0.7)


_SEG2 = ((-0.5, -0.2, 0.0), (0.4, 0.3, 0.0))


@op_geometry("segment2", 2, "P_SEGMENT2", _segment_regions(_SEG2[0][:2], _SEG2[1][:2]))
def _(ns):
    return ns.Segment(*_SEG2)


@labelled("x <= 0, y <= 0", "x > 0, y <= 0", "x >= 0, y > 0", "x < 0, y > 0")
def _rbox2_regions(l):
    x, y = l[0], l[1]
    return np.where(y > 0, np.where(x < 0, 3, 2), np.where(x > 0, 1, 0))


@op_geometry("rounded_rectangle", 2, "P_RBOX2", _rbox2_regions)
def _(ns):
    return ns.RoundedRectangle(1.0, 0.8, (0.1, 0.05, 0.2, 0.0))


_TRI = ((-0.7, -0.5, 0.0), (0.7, -0.4, 0.0), (0.0, 0.7, 0.0))


@labelled("inside", "edge 0", "edge 1", "edge 2")
def _triangle_regions(l):
    p = [np.array(v[:2]) for v in _TRI]
    e = [p[1] - p[0], p[2] - p[1], p[0] - p[2]]
    s = np.sign(e[0][0] * e[2][1] - e[0][1] * e[2][0])
    dd, cross = [], []
    for pi, ei in zip(p, e):
        v = l[:2] - pi[:, None]
        hh = np.clip(ei.dot(v) / ei.dot(ei), 0, 1)
        dd.append(np.sum((v - ei[:, None] * hh) ** 2, axis=0))
        cross.append(s * (v[0] * ei[1] - v[1] * ei[0]))
    inside = np.min(cross, axis=0) > 0
    return np.where(inside, 0, 1 + np.argmin(dd, axis=0))


@op_geometry("triangle", 2, "P_TRIANGLE2", _triangle_regions)
def _(ns):
    return ns.Triangle(*_TRI)


@op_geometry("arc2", 2, "P_ARC2", _arc_regions(0.3, 2.0))
def _(ns):
    return ns.Arc(0.6, 0.3, 2.0)


def _ngon_edge_or_vertex(l, radius, n):
    """The clip of prim_ngon on the point folded into the first sector: nearest to the edge's inside or to a vertex."""
    alpha, beta = 2 * np.pi / n, np.pi * (0.5 - 1.0 / n)
    m = np.mod(np.mod(np.arctan2(l[1], l[0]), 2 * np.pi), alpha)
    r = np.hypot(l[0], l[1])
    dot = (np.cos(m) * r - radius) * -np.cos(beta) + np.sin(m) * r * np.sin(beta)
    return ((dot <= 0) | (dot >= 2 * radius * np.sin(alpha / 2))).astype(np.int64)


@labelled(("no fold", "one fold", "two folds"), ("y >= 0", "y < 0"), ("edge", "vertex"))
def _ngon_fold_regions(l):
    alpha = 2 * np.pi / 5
    folds = np.minimum(np.floor(np.arctan2(np.abs(l[1]), l[0]) / alpha), 2).astype(np.int64)
    return np.stack([folds, (l[1] < 0).astype(np.int64), _ngon_edge_or_vertex(l, 0.5, 5)])


@op_geometry("ngon_folded", 2, "P_NGON", _ngon_fold_regions)       # integer n <= 16: the fold-count form
def _(ns):
    return ns.NGon(0.5, 5)


@labelled("edge", "vertex")
def _ngon_angle_regions(l):
    return _ngon_edge_or_vertex(l, 0.5, 18)


@op_geometry("ngon_by_angle", 2, "P_NGON", _ngon_angle_regions)    # n > 16: atan2 / mod / sincos
def _(ns):
    return ns.NGon(0.5, 18)


# -- value maps on a placed sphere --
_MAP_RADIUS = 0.6


def _sphere_value(l):
    return np.sqrt(np.sum(l * l, axis=0)) - _MAP_RADIUS


def _value_map(name, targets, apply, regions=None):
    @op_geometry(name, 3, targets, regions)
    def _(ns):
        o = ns.Sphere(_MAP_RADIUS)
        apply(ns, o)
        return o


@labelled("active", "saturated")
def _positive_regions(l):                   # v >= 0 active: VCAPEXP (e <= 1), VGAUSS clamped
    return (_sphere_value(l) < 0).astype(np.int64)


@labelled("active", "zero")
def _relu_regions(l):                       # VRELU, VSLOWSTART: max(v / w, 0)
    return (_sphere_value(l) <= 0).astype(np.int64)


@labelled("active", "saturated at 0", "saturated at 1")
def _linfall_regions(l):
    t = 1 - _sphere_value(l) / 0.5
    return np.where(t < 0, 1, np.where(t > 1, 2, 0))


_value_map("map_vsubc", "VSUBC", lambda ns, o: o.rounding(0.1))
_value_map("map_vaffine", "VAFFINE", lambda ns, o: o.rounding_cs(0.1, 1.2))
_value_map("map_vabs", "VABS", lambda ns, o: o.boundary())
_value_map("map_vneg", "VNEG", lambda ns, o: o.invert())
_value_map("map_vsign", "VSIGN", lambda ns, o: o.sign())
_value_map("map_vonion", "VONION", lambda ns, o: o.onion(0.15))
_value_map("map_vconcentric", "VCONCENTRIC", lambda ns, o: o.concentric(0.3))
_value_map("map_vsigmoid", "VSIGMOID", lambda ns, o: o.sigmoid_falloff(1.0, 0.5))
_value_map("map_vsigmoid_positive", "VSIGMOID", lambda ns, o: o.positive_sigmoid_falloff(1.0, 0.5))
_value_map("map_vcapexp", "VCAPEXP", lambda ns, o: o.capped_exponential(1.0, 0.7), _positive_regions)
_value_map("map_vhardbin", "VHARDBIN", lambda ns, o: o.hard_binarization(0.1))
_value_map("map_vlinfall", "VLINFALL", lambda ns, o: o.linear_falloff(1.0, 0.5), _linfall_regions)
_value_map("map_vrelu", "VRELU", lambda ns, o: o.relu(0.4), _relu_regions)
_value_map("map_vsmoothrelu", "VSMOOTHRELU", lambda ns, o: o.smooth_relu(0.3, 1.0, 0.05))
_value_map("map_vslowstart", "VSLOWSTART", lambda ns, o: o.slowstart(0.3, 0.5, 0.05, True), _relu_regions)
_value_map("map_vgauss_boundary", "VGAUSS", lambda ns, o: o.gaussian_boundary(1.0, 0.5))
_value_map("map_vgauss_falloff", "VGAUSS", lambda ns, o: o.gaussian_falloff(1.0, 0.5), _positive_regions)


def _expflag(ns, o):                        # default lowering: sign() of a strictly positive map folds to VEXPFLAG
    o.gaussian_falloff(1.0, 0.5)
    o.sign()


_value_map("map_vexpflag", "VEXPFLAG", _expflag)
ZERO_TANGENT_ENTRIES = ("map_vsign", "map_vhardbin", "map_vexpflag")


# -- two-value ops on two placed operands with different centres --
_CENTRES = ((-0.3, 0.1, 0.0), (0.35, -0.15, 0.2))
_RADII = (0.5, 0.4)
_RADII_SUBTRACT = (0.9, 0.8)        # the subtracted operand only wins well inside both: larger spheres


def _pair_values(l, radii):
    return [np.sqrt(np.sum((l - np.array(c)[:, None]) ** 2, axis=0)) - r for r, c in zip(radii, _CENTRES)]


def _pair(ns, radii=_RADII):
    out = []
    for r, c in zip(radii, _CENTRES):
        o = ns.Sphere(r)
        o.move(c)
        out.append(o)
    return out


def _smooth_regions(width, sa=1.0, sb=1.0, radii=_RADII):
    @labelled("blended", "first alone", "second alone")
    def regions(l):
        a, b = _pair_values(l, radii)
        a, b = sa * a, sb * b
        return np.where(width - np.abs(a - b) > 0, 0, np.where(a <= b, 1, 2))
    return regions


def _hard_regions(sa=1.0, sb=1.0, low=True, radii=_RADII):
    @labelled("first wins", "second wins")
    def regions(l):
        a, b = _pair_values(l, radii)
        a, b = sa * a, sb * b
        return ((a > b) if low else (a < b)).astype(np.int64)
    return regions


def _two_value(name, targets, operation, width=None, regions=None, radii=_RADII):
    @op_geometry(name, 3, targets, regions)
    def _(ns):
        a, b = _pair(ns, radii)
        g = ns.CombineGeometry(operation)
        return g.combine(a, b) if width is None else g.combine_parametric(a, b, parameters=width)


@op_geometry("pair_vmul", 3, "VMUL")
def _(ns):
    a, b = _pair(ns)
    a.recover_volume(b.propagate)
    return a


_two_value("pair_vadd", "VADD", "SUM")
_two_value("pair_vdiff", "VDIFF", "DIFFERENCE")
_two_value("pair_vmin", "VMIN", "UNION2", regions=_hard_regions())
_two_value("pair_vmax", "VMAX", "INTERSECT2", regions=_hard_regions(low=False))
_two_value("pair_vsubtract", "VSUBTRACT", "SUBTRACT2", regions=_hard_regions(sb=-1.0, low=False, radii=_RADII_SUBTRACT),
           radii=_RADII_SUBTRACT)
_two_value("pair_smin2", "SMIN2", "SMOOTH_UNION2_2", 0.3, _smooth_regions(0.3))
_two_value("pair_smin3", "SMIN3", "SMOOTH_UNION2", 0.3, _smooth_regions(0.3))
_two_value("pair_smax3", "SMAX3", "SMOOTH_INTERSECT2", 0.3, _smooth_regions(0.3, -1.0, -1.0))
_two_value("pair_ssub3", "SSUB3", "SMOOTH_SUBTRACT2", 0.3, _smooth_regions(0.3, -1.0, 1.0, _RADII_SUBTRACT),
           radii=_RADII_SUBTRACT)
_two_value("pair_boltz", "BOLTZ", "SMOOTH_INTERSECT2_BOLTZMANN", 0.3)
_two_value("pair_boltzsub", "BOLTZSUB", "SMOOTH_SUBTRACT2_BOLTZMANN", 0.3, radii=_RADII_SUBTRACT)


# ---- points beside the normals where two pieces of a boundary meet ------------------------------------------------------
# Beside the normal erected at a corner of the boundary, the piece with a free foot and its neighbour clipped to the
# corner are equally near to within the square of the angle to the normal, and their gradients differ by the angle. The
# points below sit at that angle on the free piece's side, where the gradient is the piece's constant normal.
NORMAL_RADII = np.geomspace(0.005, 0.5, 9)               # distance from the corner, in lengths of the free piece
NORMAL_ANGLES = np.geomspace(1e-4, 3e-3, 8)              # angle to the normal, radians


def world_coordinates(geo, local):
    """The inverse of local_coordinates: s (R local + t)."""
    R = np.asarray(geo.rotation_matrix, dtype=np.float64)
    t = np.asarray(geo.center, dtype=np.float64).reshape(3)
    return float(geo.scale) * (R.dot(local) + t[:, None])


def _beside(corner, along, normal, length):
    """corner + r (cos a * normal + sin a * along) for every radius and angle; `along` points into the free piece."""
    r, a = [x.ravel() for x in np.meshgrid(NORMAL_RADII * length, NORMAL_ANGLES)]
    return corner[:, None] + r * (np.cos(a) * normal[:, None] + np.sin(a) * along[:, None])


def triangle_normal_points():
    """Local coordinates beside both normals at every vertex of the `triangle` entry (counter-clockwise)."""
    p = [np.array(v[:2]) for v in _TRI]
    out = []
    for i in range(3):
        for j, sgn in ((i, 1.0), ((i + 2) % 3, -1.0)):      # the edge that leaves vertex i, the edge that arrives at it
            e = p[(j + 1) % 3] - p[j]
            d = e / np.linalg.norm(e)
            out.append(_beside(p[i], sgn * d, np.array([d[1], -d[0]]), np.linalg.norm(e)))
    xy = np.concatenate(out, axis=1)
    return np.concatenate([xy, np.zeros((1, xy.shape[1]))])


def cone_normal_points():
    """Local coordinates beside the two normals at the rim of the `cone` entry, the side's and the base's, at six
    azimuths. In the half plane (w0, w1) of dual_prim_cone the side runs from the apex (0, 0) to the rim q, the base from
    the axis (0, q1) to the rim."""
    h, ang = _CONE
    q = np.array([h * np.tan(ang), -h])
    d = q / np.linalg.norm(q)
    w = np.concatenate([_beside(q, -d, np.array([-d[1], d[0]]), np.linalg.norm(q)),
                        _beside(q, np.array([-1.0, 0.0]), np.array([0.0, -1.0]), q[0])], axis=1)
    phi = np.linspace(0.3, 0.3 + 2 * np.pi, 6, endpoint=False)
    z = w[1] + h * 0.5 ** (1.0 / 3.0)
    return np.concatenate([np.stack([w[0] * np.cos(f), w[0] * np.sin(f), z]) for f in phi], axis=1)


NORMAL_POINTS = {"triangle": triangle_normal_points, "cone": cone_normal_points}
