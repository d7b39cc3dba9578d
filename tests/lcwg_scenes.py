"""Liquid-crystal waveguide (LCWG) scenes shared by the golden generator (run against the REAL reference) and the tests.
Builders take the namespace under test (`spomso.cores` or `aegolius_amd.cores`) as `ns`; every array they hand to a field
is fp32-representable, so both sides see the same inputs."""
import numpy as np

f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)     # noqa: E731

# the example vector/quarter_circle_lcwg.py: inlet, quarter arc, outlet; w = width, d = thickness
U, W, D = 30, 30, 5.5
RADIUS, RUNUP, PAD = 30, 5, 5
EXAMPLE_RES = (101, 101, 51)
SMALL_RES = (21, 21, 7)            # odd along every axis: the automatic sign of LCWG2D works (co_resolution[2] odd)
# The golden keeps outputs at fixed subsets only (the fields are computed on the whole grid): it stays small.
SUBSET = 2000                      # points of the example grid kept in the golden
FIELD_PICK = 300                   # points of the small grid kept for every class x sign
SEGMENT_PICK = 500                 # points of the segment grid kept besides all of its degenerate points
CLASSES = ("LCWG2D", "LCWG3Dm1", "LCWG3Dp1")
READ_OUTS = ("create", "x", "y", "z", "phi", "theta", "length")
SLACK_READS = ("create", "phi", "theta")         # x / y / z take the rows of create's slack; length is 1 or 0
SIGN_LABELS = ("none", "float_0.1", "f64_0.2", "int_1", "int_-1", "f32_0.5", "array")
CROSSING_THR = (0.06, 0.1, 1e-3)


def read_out(vec, read):
    """What VectorField's read-outs return for the (3, N) field `vec` (reference cores/geom.py:256-362)."""
    if read == "create":
        return vec
    if read in ("x", "y", "z"):
        return vec["xyz".index(read)]
    with np.errstate(all="ignore"):
        if read == "phi":
            return np.arctan2(vec[1], vec[0])
        if read == "theta":
            return np.arccos(vec[2])
    return np.linalg.norm(vec, axis=0)


def pick(n, count, seed):
    """A fixed ascending subset of range(n)."""
    return np.sort(np.random.default_rng(seed).choice(n, min(count, n), replace=False))


def co_size():
    return (RADIUS + 2 * PAD + U / 2 + RUNUP, RADIUS + 2 * PAD + U / 2 + RUNUP, D)


def quarter_circle(ns):
    """(waveguide SDF, vertical distance) of the example, as geometry objects."""
    size = co_size()
    inlet_s = (-size[0] / 2, size[1] / 2 - W / 2 - PAD, -D / 2)
    inlet_e = (-size[1] / 2 + PAD + RUNUP, size[1] / 2 - W / 2 - PAD, -D / 2)
    outlet_s = (size[0] / 2 - PAD - W / 2, -size[1] / 2, -D / 2)
    outlet_e = (size[0] / 2 - PAD - W / 2, -size[0] / 2 + PAD + RUNUP, -D / 2)
    connection = ns.Arc(RADIUS, 0, np.pi / 2)
    connection.set_location((inlet_e[0], outlet_e[1], -D / 2))
    wg = ns.CombineGeometry("UNION").combine(ns.Segment(inlet_s, inlet_e), connection, ns.Segment(outlet_s, outlet_e))
    return wg, ns.Z(-D / 2)


def example_inputs(ns, co_resolution):
    """(uu, ww) of the example on the grid `co_resolution`, rounded to fp32."""
    coor, _ = ns.generate_grid(co_size(), co_resolution)
    wg, vertical = quarter_circle(ns)
    return f32(wg.create(coor)), f32(vertical.create(coor))


def segment_inputs(ns):
    """Straight guide along x: where the xy part of the gradient of pp vanishes, the output is +-vec by the sign of
    cos(phis) cos(2 alpha) at phis = +-pi/2 or +-3pi/2 exactly."""
    coor, res = ns.generate_grid((20, 20, 4), (41, 41, 21))
    return f32(ns.Segment((-6, 0, 0), (6, 0, 0)).create(coor)), f32(ns.Z(0).create(coor)), res


SEGMENT_WD = (8, 2)


def sign_value(label, n):
    """The `sign` argument of a label of SIGN_LABELS for n points."""
    if label == "none":
        return None
    if label == "float_0.1":
        return 0.1
    if label == "f64_0.2":
        return np.float64(0.2)
    if label == "int_1":
        return 1
    if label == "int_-1":
        return -1
    if label == "f32_0.5":
        return np.float32(0.5)
    rng = np.random.default_rng(77)
    return np.where(rng.uniform(size=n) < 0.5, -1, 1).astype(np.int64)


def field_args(cls, uu, ww):
    """(parameters, create input) of a class on the inputs."""
    if cls == "LCWG2D":
        return W, uu
    return (W, D), (uu, ww)


def old_inputs(n=1000):
    """(r, uu) of the pointwise *_old forms: positions (some on the guide's axis) and clipped distances."""
    rng = np.random.default_rng(9)
    r = f32(np.stack([rng.uniform(-20, 20, n), rng.uniform(-20, 20, n), rng.uniform(-4, 4, n)]))
    r[1:, :8] = 0.0
    return r, f32(rng.uniform(-0.5, 1.5, n))


def crossing_planes():
    """(name, plane, thr): random planes, plateaus at the minimum, thin and single-row shapes."""
    rng = np.random.default_rng(4242)
    out = []
    shapes = [(33, 29), (17, 40), (4, 4), (3, 11), (1, 23), (23, 1), (2, 7), (6, 64), (5, 130)]
    for s, shape in enumerate(shapes):
        smooth = np.sin(np.linspace(0, 5, shape[0]))[:, None] * np.cos(np.linspace(0, 7, shape[1]))[None, :] * 0.2
        random = rng.uniform(0, 0.3, size=shape)
        plateau = np.floor(rng.uniform(0, 4, size=shape)) / 16        # many points exactly at the minimum
        for kind, plane in (("smooth", smooth), ("random", random), ("plateau", plateau)):
            for thr in CROSSING_THR:
                out.append(("%s_%dx%d_%g" % (kind, shape[0], shape[1], thr), f32(plane), thr))
    return out
