"""Point-cloud and PostProcess cases shared by the golden generator (run against the REAL reference) and the tests.
Builders take the namespace under test (`spomso.cores` or `aegolius_amd.cores`) as `ns`."""
import numpy as np

f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)     # noqa: E731

SQUARE = np.asarray([[-1, -1, 0], [-1, 1, 0], [1, 1, 0], [1, -1, 0]]).T          # (3, 4): the transformation example's
ROWS3 = np.asarray([[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]])                          # 3 rows, 2 points: transposed to (2, 3)

# ---- transform chains: (name, initial points, [(method, args), ...]) -----------------------------------------------
CHAINS = [
    ("identity", SQUARE, []),
    ("example", SQUARE, [("rotate", (np.pi / 6, (0, 0, 1))), ("rescale", ((0.5, 0.75, 1),)), ("move", ((0.2, 0.1, 0),))]),
    ("rows_transposed", ROWS3, []),
    ("n_by_3", SQUARE.T.astype(float), [("move", ((1.0, 2.0, 3.0),))]),
    ("empty_list", [], []),
    ("empty_3x0", np.zeros((3, 0)), [("move", ((1.0, 0.0, 0.0),))]),
    ("single_point", np.asarray([[0.5], [0.25], [-1.0]]), [("set_scale", (2,))]),
    ("set_location_2", SQUARE, [("set_location", ((0.3, -0.2),))]),
    ("set_location_move", SQUARE, [("set_location", ((1, 2, 3),)), ("move", ((0.5, 0.5, 0.5),)), ("move", ((-1, 0, 0),))]),
    ("move_too_long", SQUARE, [("move", ((1, 2, 3, 4),))]),
    ("set_location_too_long", SQUARE, [("set_location", ((1, 2, 3, 4),))]),
    ("set_scale_float", SQUARE, [("set_scale", (1.5,))]),
    ("set_scale_vector2", SQUARE, [("set_scale", ((2.0, 3.0),))]),
    ("set_scale_bad", SQUARE, [("set_scale", ("2",))]),
    ("rescale_int", SQUARE, [("rescale", (2,))]),
    ("rescale_twice", SQUARE, [("rescale", (2,)), ("rescale", ((1.0, 0.5, 0.25),))]),
    ("rescale_vector_first", SQUARE, [("rescale", ([3.0, 2.0, 1.0],))]),
    ("rescale_bad", SQUARE, [("rescale", (None,))]),
    ("set_rotation", SQUARE, [("set_rotation", (0.7, (1, 1, 0)))]),
    ("set_rotation_np_int", SQUARE, [("set_rotation", (np.int64(1), (0, 0, 1)))]),
    ("set_rotation_axis_too_long", SQUARE, [("set_rotation", (0.5, (0, 0, 1, 0)))]),
    ("rotate_twice", SQUARE, [("rotate", (0.3, (0, 1, 0))), ("rotate", (1.1, (1, 0, 1)))]),
    ("rotate_zero_axis", SQUARE, [("rotate", (0.3, (0, 0, 0)))]),
    ("rotate_back_to_zero", SQUARE, [("rotate", (0.4, (0, 0, 1))), ("rotate", (-0.4, (0, 0, 1)))]),
    ("rotate_matrix_quirk", SQUARE, [("rotate", (np.eye(3),))]),
    ("rotate_matrix_method", SQUARE, [("rotate_matrix", (np.asarray([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0],
                                                                        [0.0, 0.0, 1.0]]),))]),
    ("rotate_three_args", SQUARE, [("rotate", (1, 2, 3))]),
    ("everything", SQUARE, [("set_scale", ((1.0, 2.0, 0.5),)), ("rotate", (0.9, (1, 2, 3))), ("set_location", ((0.1, 0.2),)),
                            ("rescale", (0.5,)), ("move", ((0.0, 0.0, 1.0),)), ("set_rotation", (0.2, (0, 0, 1)))]),
]

STATE = ("center", "scale", "rotation_matrix", "rotation_axis", "rotation_angle")


def run_chain(ns, points, steps):
    """Points(points) with the steps applied -> (object, None), or (object or None, exception type name)."""
    try:
        p = ns.Points(points)
    except Exception as exc:  # noqa: BLE001
        return None, type(exc).__name__
    for method, args in steps:
        try:
            getattr(p, method)(*args)
        except Exception as exc:  # noqa: BLE001
            return p, type(exc).__name__
    return p, None


# ---- to_image cases: (name, cloud (3, N), co_size, co_resolution, extend) ------------------------------------------
def _image_clouds():
    rng = np.random.default_rng(7)
    edges = np.linspace(-1.0, 1.0, 10)            # the edges of 9 bins on [-1, 1]
    on_edges = np.stack(np.meshgrid(edges, edges[::2], edges[1::3], indexing="ij")).reshape(3, -1)
    special = np.asarray([[np.nan, 0.1, 0.1], [0.1, np.nan, 0.1], [0.1, 0.1, np.nan], [np.inf, 0.0, 0.0],
                          [-np.inf, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf], [1.0, 1.0, 1.0],
                          [-1.0, -1.0, -1.0], [1.0000001, 0.0, 0.0], [0.0, -1.0000001, 0.0], [0.2, 0.3, 0.4]]).T
    blob = rng.normal(0.0, 0.35, (3, 400))
    flat = np.concatenate([rng.uniform(-0.8, 0.8, (2, 300)), np.zeros((1, 300))])
    corner = np.asarray([[-0.95, 0.9], [0.9, -0.95], [-0.2, 0.1]])
    return {"on_edges": on_edges, "special": special, "blob": blob, "flat": flat, "corner": corner,
            "empty": np.zeros((3, 0))}


ALL6 = ("-X", "+X", "-Y", "+Y", "-Z", "+Z")
TO_IMAGE = [
    ("on_edges", "on_edges", (2, 2, 2), (9, 9, 9), ()),
    ("on_edges_even_res", "on_edges", (2, 2, 2), (8, 10, 4), ()),
    ("special", "special", (2, 2, 2), (9, 9, 9), ()),
    ("special_all6", "special", (2, 2, 2), (9, 9, 9), ALL6),
    ("outside", "blob", (1, 1, 1), (15, 15, 15), ()),
    ("blob_65", "blob", (2.5, 2.5, 2.5), (65, 65, 65), ()),
    ("blob_aniso", "blob", (3, 2, 1), (33, 21, 9), ()),
    ("zero_size_z", "flat", (2, 2, 0), (17, 17, 1), ()),
    ("zero_size_z_res5", "flat", (2, 2, 0), (17, 17, 5), ("-Z", "+Z")),
    ("flat_z0", "flat", (2, 2, 2), (17, 17, 17), ()),
    ("flat_z0_zz", "flat", (2, 2, 2), (17, 17, 17), ("-Z", "+Z")),
    ("flat_z0_zzx", "flat", (2, 2, 2), (17, 17, 17), ("-Z", "+Z", "-X")),
    ("corner_mx", "corner", (2, 2, 2), (21, 21, 21), ("-X",)),
    ("corner_px", "corner", (2, 2, 2), (21, 21, 21), ("+X",)),
    ("corner_my", "corner", (2, 2, 2), (21, 21, 21), ("-Y",)),
    ("corner_py", "corner", (2, 2, 2), (21, 21, 21), ("+Y",)),
    ("corner_mz", "corner", (2, 2, 2), (21, 21, 21), ("-Z",)),
    ("corner_pz", "corner", (2, 2, 2), (21, 21, 21), ("+Z",)),
    ("corner_all6", "corner", (2, 2, 2), (21, 21, 21), ALL6),
    ("corner_all6_reversed", "corner", (2, 2, 2), (21, 21, 21), ALL6[::-1]),
    ("corner_repeated", "corner", (2, 2, 2), (21, 21, 21), ("-X", "-X", "+Z", "-X", "+Z")),
    ("corner_unknown", "corner", (2, 2, 2), (21, 21, 21), ("X", "+W", "-z", "+Y")),
    ("corner_string", "corner", (2, 2, 2), (21, 21, 21), "-Z"),
    ("blob_all6", "blob", (2, 2, 2), (31, 25, 19), ALL6),
    ("blob_mixed", "blob", (2, 2, 2), (31, 25, 19), ("+Y", "-Z", "-X", "+Z")),
    ("empty_no_extend", "empty", (2, 2, 2), (9, 9, 9), ()),
    ("empty_extend", "empty", (2, 2, 2), (9, 9, 9), ("-Z",)),
    ("empty_unknown", "empty", (2, 2, 2), (9, 9, 9), ("up",)),
    ("outside_extend", "blob", (0.01, 0.01, 0.01), (5, 5, 5), ("+X",)),
    ("negative_range", "blob", (-2, 2, 2), (9, 9, 9), ()),
    ("negative_res", "blob", (2, 2, 2), (9, -3, 9), ()),
    ("infinite_range", "blob", (2, np.inf, 2), (9, 9, 9), ()),
    ("two_dim_cloud", "flat2d", (2, 2, 2), (9, 9, 9), ()),
]


def image_cloud(name):
    if name == "flat2d":
        return _image_clouds()["flat"][:2]
    return _image_clouds()[name]


def to_image_case(ns, case):
    """The reference's Points(cloud).to_image -> (grid, None) or (None, exception type name)."""
    _name, cloud, size, res, extend = case
    p = ns.Points(np.zeros((3, 0)))
    p._points = image_cloud(cloud)             # the cloud as given (Points() would transpose a 2 x 300 cloud wrongly)
    try:
        return p.to_image(size, res, extend), None
    except Exception as exc:  # noqa: BLE001
        return None, type(exc).__name__


def to_image_restated(cloud, size, res, extend):
    """numpy.histogramdd(...) > 0 with the reference's extend fills restated: the test's independent model."""
    res = tuple(int(r if r % 2 == 1 else r + 1) for r in res)
    out, _ = np.histogramdd(np.asarray(cloud).T, bins=res, range=[(-s / 2, s / 2) for s in size])
    out = (out > 0).astype(float)
    for ex in extend:
        if ex not in ALL6:
            continue
        axis = "XYZ".index(ex[1])
        occupied = np.flatnonzero(np.moveaxis(out, axis, 0).reshape(res[axis], -1).max(axis=1) > 0)
        view = np.moveaxis(out, axis, 0)
        if ex[0] == "-":
            view[:occupied[0]] = view[occupied[0]]
        else:
            view[occupied[-1] + 1:] = view[occupied[-1]]
    return out


# ---- PostProcess ---------------------------------------------------------------------------------------------------
PP_SIZE, PP_RES = (4, 4), (48, 48)          # 49 x 49 after resolution_conversion


def sinc(u, amplitude, width):
    return amplitude * np.sinc(u / width)


def pp_methods(res):
    """(label, method, args) of each of the 13 PostProcess methods; res: the grid resolution of the conv methods."""
    return [
        ("sigmoid_falloff", "sigmoid_falloff", (1.0, 0.5)),
        ("positive_sigmoid_falloff", "positive_sigmoid_falloff", (1.0, 0.5)),
        ("capped_exponential", "capped_exponential", (1, 0.5)),
        ("hard_binarization", "hard_binarization", (0.05,)),
        ("linear_falloff", "linear_falloff", (1.0, 0.5)),
        ("relu", "relu", (0.7,)),
        ("smooth_relu", "smooth_relu", (0.3, 1.5, 0.02)),
        ("slowstart", "slowstart", (0.3, 1, 0.01, False)),
        ("gaussian_boundary", "gaussian_boundary", (1.0, 0.5)),
        ("gaussian_falloff", "gaussian_falloff", (1.0, 0.5)),
        ("conv_averaging", "conv_averaging", (3, 2, res)),
        ("conv_edge_detection", "conv_edge_detection", (res,)),
        ("Sinc", "custom_post_process", (sinc, (1.0, 0.5), "Sinc")),
    ]


def pp_field(ns, method, args, co):
    """PostProcess(Circle(1).propagate).<method>(*args), evaluated through GenericGeometry(..., ()).create(co)."""
    circle = ns.Circle(1)
    pp = ns.PostProcess(circle.propagate)
    getattr(pp, method)(*args)
    return ns.GenericGeometry(pp.processed_geo_object, ()).create(co), pp


def pp_chain_field(ns, co):
    """A chain of three steps on a bare sdf function whose parameter is passed at call time."""
    pp = ns.PostProcess(ns.sdf_circle)
    pp.relu(0.5)
    pp.smooth_relu(0.2)
    pp.capped_exponential(2.0, 0.75)
    return ns.GenericGeometry(pp.processed_geo_object, 0.8).create(co), pp


# ---- the example scripts -------------------------------------------------------------------------------------------
def points_transformations_2d(ns, co):
    """2D/points_transformations_2D.py: final_pattern."""
    points = ns.Points(SQUARE)
    points.rotate(np.pi / 6, (0, 0, 1))
    points.rescale((0.5, 0.75, 1))
    points.move((0.2, 0.1, 0))
    final = ns.PointCloud2D(points.cloud)
    final.onion(0.1)
    return final.create(co)


OOP_STEPS = (("ce", "capped_exponential", (1, 0.5)), ("rl", "relu", (1.0,)), ("gb", "gaussian_boundary", (1.0, 0.5)),
             ("lf", "linear_falloff", (1.0, 0.5)), ("sf", "sigmoid_falloff", (1.0, 0.5)),
             ("gf", "gaussian_falloff", (1.0, 0.5)), ("hb", "hard_binarization", (0,)))


def post_processing_oop_2d(ns, co):
    """2D/post_processing_scalar_oop_2D.py: the seven `<key>_geo_field` arrays."""
    final = ns.Circle(1)
    out = {}
    for key, method, args in OOP_STEPS:
        pp = ns.PostProcess(final.propagate)
        getattr(pp, method)(*args)
        out[key] = ns.GenericGeometry(pp.processed_geo_object, ()).create(co)
    return out


def approaches_oop_2d(ns, co):
    """2D/approaches_post_processing_scalar_2D.py: gb_geo_field (the PostProcess variant)."""
    pp = ns.PostProcess(ns.Circle(1).propagate)
    pp.gaussian_boundary(1.0, 0.5)
    return ns.GenericGeometry(pp.processed_geo_object, ()).create(co)


def custom_oop_2d(ns, co):
    """2D/custom_post_processing_scalar_2D.py: custom_geo_field (the PostProcess variant)."""
    pp = ns.PostProcess(ns.Circle(1).propagate)
    pp.custom_post_process(sinc, (1.0, 0.5), post_process_name="Sinc")
    return ns.GenericGeometry(pp.processed_geo_object, ()).create(co)


# (script, its (co_size, co_resolution), the builder, script variable(s) -> builder output key)
SCRIPTS = [
    ("2D/points_transformations_2D.py", ((3, 3), (400, 400)), points_transformations_2d, {"final_pattern": None}),
    ("2D/post_processing_scalar_oop_2D.py", ((4, 4), (400, 400)), post_processing_oop_2d,
     {"%s_geo_field" % k: k for k, _m, _a in OOP_STEPS}),
    ("2D/approaches_post_processing_scalar_2D.py", ((4, 4), (400, 400)), approaches_oop_2d, {"gb_geo_field": None}),
    ("2D/custom_post_processing_scalar_2D.py", ((4, 4), (400, 400)), custom_oop_2d, {"custom_geo_field": None}),
]
SCRIPT_SMALL_RES = (100, 100)
