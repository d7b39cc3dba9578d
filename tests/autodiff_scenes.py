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
