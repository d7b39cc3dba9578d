"""Points, EuclideanTransformPoints and PostProcess without a GPU: the reference's signatures, the transform chains and
from_image bit for bit against fixtures recorded from the real reference (tests/golden/generate_points_golden.py), the
checks of to_image that raise before any device call, and the PostProcess lowering (one fused program, the same as the
equivalent ModifyObject chain; the float64 oracle reproduces its fields)."""
import inspect
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import aegolius_amd.cores as ns  # noqa: E402
import points_scenes as S  # noqa: E402
from aegolius_amd import _points  # noqa: E402
from aegolius_amd._lower import lower_geometry  # noqa: E402
from oracle import sdf_oracle  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "points_golden_meta.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, "points_golden.npz"))


def _params(obj):
    return [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
            for p in inspect.signature(obj).parameters.values()]


@pytest.mark.parametrize("mod_name, name", [("geom", "Points"), ("transformations", "EuclideanTransformPoints"),
                                            ("post_processing", "PostProcess")])
def test_signatures_match_the_reference(mod_name, name):
    import importlib
    with open(os.path.join(GOLDEN, "reference_api.json")) as f:
        want = json.load(f)["modules"][mod_name][name]
    cls = getattr(importlib.import_module("aegolius_amd.cores." + mod_name), name)
    assert [b.__name__ for b in cls.__bases__ if b is not object] == want["bases"]
    assert _params(cls) == want["signature"]
    for meth, sig in want["methods"].items():
        assert _params(getattr(cls, meth)) == sig, meth
    for prop in want["properties"]:
        assert isinstance(inspect.getattr_static(cls, prop), property), prop
    assert getattr(ns, name) is cls


@pytest.mark.parametrize("name, points, steps", S.CHAINS, ids=[c[0] for c in S.CHAINS])
def test_transform_chain_matches_the_reference(name, points, steps, golden):
    meta, arrays = golden
    rec = meta["chains"][name]
    p, err = S.run_chain(ns, points, steps)
    assert err == rec["error"]
    assert (list(p.transformations) if p is not None else None) == rec["labels"]
    if p is None:
        return
    for attr in S.STATE:
        v = getattr(p, attr)
        assert type(v).__name__ == rec[attr + "_type"], attr
        want = arrays["chain_%s_%s" % (name, attr)]
        assert np.asarray(v).shape == want.shape and np.array_equal(np.asarray(v), want, equal_nan=True), attr
    if err is None:
        if rec["cloud_error"] is None:
            got = p.cloud
            want = arrays["chain_%s_cloud" % name]
            assert got.dtype == want.dtype and got.shape == want.shape
            assert np.array_equal(got.view(np.uint64) if got.size else got, want.view(np.uint64) if want.size else want)
        else:
            with pytest.raises(Exception) as info:
                p.cloud
            assert type(info.value).__name__ == rec["cloud_error"]


def test_center_and_scale_state_semantics():
    p = ns.Points(S.SQUARE)
    c = p.center
    p.move((1, 2, 3))
    p.set_location((5,))
    assert c is p.center and np.array_equal(c, [5.0, 2.0, 3.0])          # updated in place
    assert p.scale == 1.0 and isinstance(p.scale, float)
    p.rescale(2)
    assert isinstance(p.scale, np.ndarray) and np.array_equal(p.scale, [2.0, 2.0, 2.0])
    with pytest.raises(TypeError):
        ns.EuclideanTransformPoints.get_rotation_matrix(np.int32(1), (0, 0, 1))


def _alpha_greyscale(la):
    a = la / 255.0
    return np.maximum(1 - a[:, :, 1], a[:, :, 0])


def test_from_image_reproduces_the_image_clouds():
    px = np.load(os.path.join(GOLDEN, "image_pixels.npz"))
    want = np.load(os.path.join(GOLDEN, "image_clouds.npz"))
    owl = _alpha_greyscale(px["owl"])
    shapes = _alpha_greyscale(px["shapes"])
    cases = {"lines": (px["lines"], (3, 1.5), 0.5), "owl_exterior": (owl, (9, 16), 0.0),
             "owl_interior": (1 - owl, (9, 16), 0.0), "shapes": (shapes, (3, 1.5), 0.2)}
    for key, (image, size, threshold) in cases.items():
        p = ns.Points([])
        p.from_image(image, size, binary_threshold=threshold)
        c = p.cloud
        assert c.shape[0] == 3 and not c[2].any(), key
        assert np.array_equal(c[:2].view(np.uint64), want[key].view(np.uint64)), key


@pytest.fixture
def no_gpu(monkeypatch):
    """Any device call fails the test."""
    def refuse(*_a, **_k):
        raise AssertionError("to_image reached the device before its inputs were checked")
    monkeypatch.setattr(_points._engine, "require_gpu", refuse)
    monkeypatch.setattr(_points._engine, "lib", refuse)


@pytest.mark.parametrize("case", [c for c in S.TO_IMAGE if c[0] in ("negative_range", "negative_res", "infinite_range",
                                                                    "two_dim_cloud")], ids=lambda c: c[0])
def test_to_image_rejects_bad_input_before_the_device(case, golden, no_gpu):
    grid, err = S.to_image_case(ns, case)
    assert grid is None and err == golden[0]["to_image"][case[0]]["error"]


def test_to_image_checks_like_numpy(no_gpu):
    cloud = np.zeros((3, 4))
    with pytest.raises(ValueError, match="dimension of bins"):
        _points.to_image(np.zeros((2, 4)), (1, 1, 1), (3, 3, 3), ())
    with pytest.raises(ValueError, match="max must be larger"):
        _points.to_image(cloud, (1, -1, 1), (3, 3, 3), ())
    with pytest.raises(ValueError, match="not finite"):
        _points.to_image(cloud, (1, 1, np.nan), (3, 3, 3), ())
    with pytest.raises(ValueError, match="must be positive"):
        _points.to_image(cloud, (1, 1, 1), (3, -1, 3), ())
    with pytest.raises(TypeError):
        _points.to_image(cloud, (1, 1, 1), (3, 3, 3), None)
    with pytest.raises(IndexError):
        _points.to_image(cloud, (1, 1), (3, 3, 3), ())


def test_edges_are_numpys():
    sample, res, edges, entries = _points.prepare(np.zeros((3, 2)), (2.2, 0, 3), (8, 1, 7), ("-Z", "up"))
    assert res == (9, 1, 7) and entries == ["-Z", "up"] and sample.flags.c_contiguous and sample.dtype == np.float64
    for e, size, n in zip(edges, (2.2, 0, 3), res):
        _, want = np.histogram(np.zeros(0), bins=n, range=(-size / 2, size / 2))
        assert np.array_equal(e, want)


def test_post_process_labels_and_structure():
    circle = ns.Circle(1)
    pp = ns.PostProcess(circle.propagate)
    assert pp.unprocessed_object is pp.unprocessed_geo_object and pp.processed_object is pp.processed_geo_object
    assert pp.post_processing_operations == []
    for label, method, args in S.pp_methods((5, 5)):
        before = pp.processed_geo_object
        step = getattr(pp, method)(*args)
        assert step is pp.processed_geo_object and step is pp.processed_object and step is not before
        assert callable(step) and step.inner is not None
        assert pp.post_processing_operations[-1] == label
    assert pp.post_processing_operations == [m[0] for m in S.pp_methods((5, 5))]
    assert pp.unprocessed_geo_object == circle.propagate


POINTWISE = [m for m in S.pp_methods(S.PP_RES) if m[1] not in ("conv_averaging", "conv_edge_detection",
                                                                   "custom_post_process")]


@pytest.mark.parametrize("label, method, args", POINTWISE, ids=[m[0] for m in POINTWISE])
def test_post_process_program_is_the_modify_object_program(label, method, args):
    circle = ns.Circle(1)
    pp = ns.PostProcess(circle.propagate)
    getattr(pp, method)(*args)
    got = lower_geometry(ns.GenericGeometry(pp.processed_geo_object, ()))
    mod = ns.Circle(1)
    getattr(mod, method)(*args)
    want = lower_geometry(mod)
    assert np.array_equal(got.code, want.code) and np.array_equal(got.params, want.params)
    assert got.result_reg == want.result_reg


def test_post_process_chain_with_call_time_parameters_is_one_program():
    pp = ns.PostProcess(ns.sdf_circle)
    pp.relu(0.5)
    pp.smooth_relu(0.2)
    pp.capped_exponential(2.0, 0.75)
    got = lower_geometry(ns.GenericGeometry(pp.processed_geo_object, 0.8))
    mod = ns.GenericGeometry(ns.sdf_circle, 0.8)
    mod.relu(0.5)
    mod.smooth_relu(0.2)
    mod.capped_exponential(2.0, 0.75)
    want = lower_geometry(mod)
    assert np.array_equal(got.code, want.code) and np.array_equal(got.params, want.params)


def test_oracle_reproduces_the_post_process_goldens(golden):
    meta, arrays = golden
    co, _ = ns.generate_grid(S.PP_SIZE, S.PP_RES)
    co = S.f32(co)
    for label, method, args in S.pp_methods(S.PP_RES):
        circle = ns.Circle(1)
        pp = ns.PostProcess(circle.propagate)
        getattr(pp, method)(*args)
        got = sdf_oracle.evaluate(ns.GenericGeometry(pp.processed_geo_object, ()), co)
        want = arrays["pp_%s" % label]
        assert list(got.shape) == meta["post_process"][label]["shape"] == list(want.shape), label
        assert np.allclose(got, want, rtol=0, atol=1e-12), label
    pp = ns.PostProcess(ns.sdf_circle)
    pp.relu(0.5)
    pp.smooth_relu(0.2)
    pp.capped_exponential(2.0, 0.75)
    got = sdf_oracle.evaluate(ns.GenericGeometry(pp.processed_geo_object, 0.8), co)
    assert np.allclose(got, arrays["pp_chain"], rtol=0, atol=1e-12)
