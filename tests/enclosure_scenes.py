"""Scenes of the enclosure tests (tests/test_enclosure_cpu.py, tests/test_gpu_enclosure.py): name -> (builder(ns), domain
sizes). Every builder takes the namespace that provides the operator API, as aegolius_amd.workloads does.

  * the five BASELINE configs,
  * one Box (a Rectangle where the modification is 2-D) under each single modification that has a coordinate rule,
  * a twisted half space whose normal lies between the tangential and the z direction, and a sheared Box twisted: the
    directions in which a twist stretches most, which a Box aligned with the axes never probes,
  * one tree per value operation and per combiner; the product (VMUL) comes with the signed regions: a polygon and a
    closed curve's shape (distance to the outline times a sign primitive), alone and in a union, where the lowering
    copies the coordinate register first (MOVC).
"""
import numpy as np

from aegolius_amd import workloads


def _box(ns):
    return ns.Box(0.6, 0.3, 0.2)


def _mod(method, *args, base=_box, pre=None):
    def build(ns):
        b = base(ns)
        if pre is not None:
            pre(b)
        getattr(b, method)(*args)
        return b
    return build


def _rect(ns):
    return ns.Rectangle(0.4, 0.3)


def _rotated(ns):
    b = _box(ns)
    b.rotate(0.7, (1, 2, 3))
    b.move((0.3, -0.2, 0.1))
    return b


def _moved(b):
    b.move((0.25, 0.1, -0.05))


def _pair(ns):
    a = ns.Sphere(0.45)
    a.move((0.2, 0.1, -0.1))
    b = _rotated(ns)
    return a, b


def _combine(op, parameter=None):
    def build(ns):
        a, b = _pair(ns)
        if parameter is None:
            return ns.CombineGeometry(op).combine(a, b)
        return ns.CombineGeometry(op).combine_parametric(a, b, parameters=parameter)
    return build


def _twisted_plane(ns):
    p = ns.OrientedPlane((0, 2, 1), 0)
    p.twist(np.pi / 2)
    return p


def _sheared_twisted(ns):
    # lowers to XLATE, TWIST, LIN3, P_BOX: the shear between y and z tilts the Box's faces inside the twisted frame
    b = _box(ns)
    _moved(b)
    b.shear_yz(0.8)
    b.twist(np.pi / 2)
    return b


def _polygon(ns):
    # a simple, concave outline (counter-clockwise), no edge on a dyadic line
    pts = np.array([[-0.52, 0.47, 0.51, 0.13, 0.09, -0.48], [-0.41, -0.43, 0.12, 0.08, 0.46, 0.44], [0.0] * 6])
    line = ns.SegmentedLine(pts, closed=True)
    line.polygon()
    return line


def _ellipse(t, a, b):
    return np.asarray((a * np.cos(t), b * np.sin(t)))


def _shape(ns):
    curve = ns.ParametricCurve(_ellipse, (0.6, 0.35), (0, 2 * np.pi, 24), closed=True)
    curve.shape()
    return curve


def _polygon_union(ns):
    a = _polygon(ns)
    b = ns.Circle(0.3)
    b.move((0.45, 0.3, 0))
    return ns.CombineGeometry("UNION2").combine(a, b)


def _flag(ns):
    b = _rotated(ns)
    b.gaussian_falloff(1.0, 0.5)
    b.sign()
    return b


BASELINE = {
    "cfg1": (workloads.cfg1_sphere, (2, 2, 2)),
    "cfg2": (workloads.cfg2_tree, (2, 2, 2)),
    "cfg3": (workloads.cfg3_chain, (4, 4, 4)),
    "cfg4": (workloads.cfg4_scene2d, (10, 10)),
    "cfg5": (workloads.cfg5_tree, (3, 3, 3)),
}
FINITE_L = ("cfg1", "cfg2", "cfg4", "cfg5")

MODS = {
    "move": (_mod("move", (0.3, -0.2, 0.1)), (3, 3, 3)),
    "rotate": (_rotated, (3, 3, 3)),
    "shear": (_mod("shear_xz", 0.4), (3, 3, 3)),
    "scale": (_mod("rescale", 1.5), (3, 3, 3)),
    "rounding_cs": (_mod("rounding_cs", 0.05, 0.6), (3, 3, 3)),
    "elongation": (_mod("elongation", (0.4, 0.0, 0.1)), (3, 3, 3)),
    "revolution": (_mod("revolution", 0.7, base=_rect), (3, 3, 3)),
    "axis_revolution": (_mod("axis_revolution", 0.7, 0.5, base=_rect), (3, 3, 3)),
    "extrusion": (_mod("extrusion", 0.4, base=_rect), (3, 3, 3)),
    "twist": (_mod("twist", np.pi / 2, pre=_moved), (3, 3, 3)),
    "bend": (_mod("bend", 1.5, np.pi / 3), (4, 4, 4)),
    "infinite_repetition": (_mod("infinite_repetition", (1.5, 1.0, 2.0)), (4, 4, 4)),
    "finite_repetition": (_mod("finite_repetition", (3.0, 2.0, 1.0), (3, 2, 1)), (4, 4, 4)),
    "symmetry": (_mod("symmetry", 0, pre=_moved), (3, 3, 3)),
    "mirror": (_mod("mirror", (-0.5, 0.1, 0.0), (0.7, -0.2, 0.3), pre=_moved), (3, 3, 3)),
    "rotational_symmetry": (_mod("rotational_symmetry", 5, 0.6, 0.2), (3, 3, 3)),
    "linear_instancing": (_mod("linear_instancing", 4, (-1.0, 0.0, 0.0), (1.0, 0.5, 0.0)), (4, 4, 4)),
    "twisted_plane": (_twisted_plane, (3, 3, 3)),
    "sheared_box_twisted": (_sheared_twisted, (3, 3, 3)),
}

VALUES = {
    "rounding": (_mod("rounding", 0.05, base=_rotated), (3, 3, 3)),
    "boundary": (_mod("boundary", base=_rotated), (3, 3, 3)),
    "invert": (_mod("invert", base=_rotated), (3, 3, 3)),
    "sign": (_mod("sign", base=_rotated), (3, 3, 3)),
    "onion": (_mod("onion", 0.04, base=_rotated), (3, 3, 3)),
    "concentric": (_mod("concentric", 0.1, base=_rotated), (3, 3, 3)),
    "sigmoid_falloff": (_mod("sigmoid_falloff", 1.5, 0.3, base=_rotated), (3, 3, 3)),
    "positive_sigmoid_falloff": (_mod("positive_sigmoid_falloff", 1.5, 0.3, base=_rotated), (3, 3, 3)),
    "capped_exponential": (_mod("capped_exponential", 2.0, 0.4, base=_rotated), (3, 3, 3)),
    "hard_binarization": (_mod("hard_binarization", 0.1, base=_rotated), (3, 3, 3)),
    "linear_falloff": (_mod("linear_falloff", 1.2, 0.5, base=_rotated), (3, 3, 3)),
    "relu": (_mod("relu", 0.5, base=_rotated), (3, 3, 3)),
    "smooth_relu": (_mod("smooth_relu", 0.1, 0.5, base=_rotated), (3, 3, 3)),
    "slowstart": (_mod("slowstart", 0.1, 0.5, base=_rotated), (3, 3, 3)),
    "gaussian_boundary": (_mod("gaussian_boundary", 1.0, 0.5, base=_rotated), (3, 3, 3)),
    "gaussian_falloff": (_mod("gaussian_falloff", 1.0, 0.5, base=_rotated), (3, 3, 3)),
    "gaussian_flag": (_flag, (3, 3, 3)),
}

COMBINERS = {
    "UNION2": (_combine("UNION2"), (3, 3, 3)),
    "SUBTRACT2": (_combine("SUBTRACT2"), (3, 3, 3)),
    "INTERSECT2": (_combine("INTERSECT2"), (3, 3, 3)),
    "SUM": (_combine("SUM"), (3, 3, 3)),
    "DIFFERENCE": (_combine("DIFFERENCE"), (3, 3, 3)),
    "SMOOTH_UNION2_2": (_combine("SMOOTH_UNION2_2", 0.15), (3, 3, 3)),
    "SMOOTH_UNION2": (_combine("SMOOTH_UNION2", 0.15), (3, 3, 3)),
    "SMOOTH_INTERSECT2": (_combine("SMOOTH_INTERSECT2", 0.15), (3, 3, 3)),
    "SMOOTH_SUBTRACT2": (_combine("SMOOTH_SUBTRACT2", 0.15), (3, 3, 3)),
    "SMOOTH_INTERSECT2_BOLTZMANN": (_combine("SMOOTH_INTERSECT2_BOLTZMANN", 0.15), (3, 3, 3)),
    "SMOOTH_SUBTRACT2_BOLTZMANN": (_combine("SMOOTH_SUBTRACT2_BOLTZMANN", 0.15), (3, 3, 3)),
    "polygon": (_polygon, (2, 2)),                    # P_SEGLINE2, P_POLYSIGN, VMUL
    "shape": (_shape, (2, 2)),                        # P_NEAREST2, P_SHAPESIGN, VMUL
    "polygon_union": (_polygon_union, (2, 2)),        # the same after MOVC
}

SCENES = {}
for _group in (BASELINE, MODS, VALUES, COMBINERS):
    SCENES.update(_group)


def special_locations(name, size):
    """Points a box of the scene should straddle: per axis, coordinates of the planes x = 0 / y = 0 / z = 0, repetition cell
    borders, the end of the bent arc, the cut of atan2 (the negative x axis: y = 0 again) -> list of (3,) centres."""
    pts = [(0.0, 0.0, 0.0), (0.3, 0.0, 0.2), (0.0, -0.4, 0.1), (-0.5, 0.2, 0.0), (-0.7, 0.0, 0.3)]
    if name in ("cfg3", "infinite_repetition"):
        pts += [(1.0, 0.2, 0.1), (0.75, 0.5, 1.0), (0.2, 1.0, -1.0), (-1.0, -1.0, 1.0), (0.75, 0.1, 0.3)]
    if name in ("cfg3", "bend"):
        R, a = 1.5, np.pi / 3
        pts += [(R * np.sin(a / 2), R * (1 - np.cos(a / 2)), 0.0), (-R * np.sin(a / 2), R * (1 - np.cos(a / 2)), 0.1),
                (0.0, R, 0.0), (0.0, 1.9, 0.0), (1e-3, 1.9, 0.0)]
    if name == "finite_repetition":
        pts += [(0.5, 0.0, 0.0), (-0.5, 0.0, 0.0), (1.5, 1.0, 0.5), (0.5, 0.0, 0.25)]
    if name == "linear_instancing":
        pts += [(0.33, 0.17, 0.0), (-0.6, -0.3, 0.0), (0.9, 0.45, 0.1)]
    if name == "rotational_symmetry":
        ang = 2 * np.pi / 5
        pts += [(0.8 * np.cos(k * ang + 0.2 - ang / 2), 0.8 * np.sin(k * ang + 0.2 - ang / 2), 0.0) for k in range(5)]
    half = [s / 2.0 for s in size]
    return [p for p in pts if all(abs(p[a]) < half[a] for a in range(len(size)))]


def boxes(name, size, count, seed=0):
    """`count` boxes (float32 ends, (3, count); z = 0 for a 2-D scene) in and around the domain of `size`: degenerate
    ones, half widths log-uniform from 1e-6 to the domain size, the whole domain, boxes straddling the special locations
    of the scene (at four half widths) and one tall enough for a twist to turn more than once across it."""
    rng = np.random.default_rng(seed)
    dims = len(size)
    half = np.array([s / 2.0 for s in size])
    lo, hi = [], []

    def add(c, h):
        c, h = np.asarray(c, dtype=np.float64)[:dims], np.broadcast_to(np.asarray(h, dtype=np.float64), (dims,))
        lo.append(c - h)
        hi.append(c + h)

    add(np.zeros(dims), half)                                             # the whole domain
    add(np.zeros(dims), np.concatenate([half[:dims - 1] * 0.1, [max(5.0, half[-1])]]))   # tall: > one turn of a twist
    for p in special_locations(name, size):
        for h in (0.0, 1e-4, 0.05, 0.4):
            add(p, h)
    k = 0
    while len(lo) < count:
        c = rng.uniform(-half, half)
        if k % 8 == 0:
            add(c, 0.0)                                                   # degenerate
        else:
            add(c, np.exp(rng.uniform(np.log(1e-6), np.log(float(max(size))), dims)))
        k += 1
    lo64, hi64 = np.array(lo[:count]).T, np.array(hi[:count]).T
    lo32, hi32 = lo64.astype(np.float32), hi64.astype(np.float32)
    if dims == 2:
        z = np.zeros((1, lo32.shape[1]), dtype=np.float32)
        lo32, hi32 = np.concatenate([lo32, z]), np.concatenate([hi32, z])
    return np.ascontiguousarray(lo32), np.ascontiguousarray(hi32)


def sample_points(lo32, hi32, per_box=64, seed=1):
    """`per_box` float32 points of every box: its 8 corners, its centre and random ones, clipped into the box ->
    (3, n * per_box) float32, box k at columns k * per_box ..."""
    rng = np.random.default_rng(seed)
    n = lo32.shape[1]
    lo, hi = lo32.astype(np.float64), hi32.astype(np.float64)
    t = rng.uniform(0.0, 1.0, (3, n, per_box))
    for k in range(8):
        t[0, :, k], t[1, :, k], t[2, :, k] = k & 1, (k >> 1) & 1, k >> 2
    t[:, :, 8] = 0.5
    p = (lo[:, :, None] + t * (hi - lo)[:, :, None]).astype(np.float32)
    p = np.minimum(np.maximum(p, lo32[:, :, None]), hi32[:, :, None])
    return np.ascontiguousarray(p.reshape(3, n * per_box))
