"""Points.to_image on the GPU (csrc/sdfk_points.inc) and PostProcess fields, against fixtures recorded from the real
reference (tests/golden/generate_points_golden.py) and against numpy.histogramdd with the extend fills restated."""
import ctypes
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
from aegolius_amd import _engine, _points  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "points_golden_meta.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, "points_golden.npz"))


def _unpack(arrays, name, shape):
    bits = np.unpackbits(arrays["image_%s" % name], count=int(np.prod(shape)))
    return bits.reshape(shape).astype(np.float64)


class _Resident:
    """Points.to_image through to_image_resident, read back to the host for comparison."""

    class _P(ns.Points):
        def to_image(self, co_size, co_resolution, extend):
            dev = self.to_image_resident(co_size, co_resolution, extend)
            try:
                v = dev.numpy()
            finally:
                dev.free()
            assert v.dtype == np.float32
            res = tuple(ns.resolution_conversion(r) for r in co_resolution)
            return v.astype(np.float64).reshape(res)

    def __getattr__(self, name):
        return self._P if name == "Points" else getattr(ns, name)


@pytest.mark.parametrize("via", ["bytes", "f64", "resident"])
def test_every_to_image_case_matches_the_reference(via, golden, monkeypatch):
    meta, arrays = golden
    monkeypatch.setattr(_points, "DEFAULT_TRANSFER", "f64" if via == "f64" else "bytes")
    space = _Resident() if via == "resident" else ns
    for case in S.TO_IMAGE:
        rec = meta["to_image"][case[0]]
        grid, err = S.to_image_case(space, case)
        assert err == rec["error"], case[0]
        if err is None:
            want = _unpack(arrays, case[0], tuple(rec["shape"]))
            assert grid.dtype == np.float64 and grid.shape == want.shape and grid.flags.c_contiguous, case[0]
            assert np.array_equal(grid, want), case[0]


def test_random_clouds_against_histogramdd():
    rng = np.random.default_rng(11)
    for trial in range(12):
        n = int(rng.integers(10, 20000))
        cloud = rng.normal(0, 0.6, (3, n))
        cloud[:, rng.integers(0, n, 5)] = np.round(cloud[:, :5] * 8) / 8           # some points on edges
        size = tuple(rng.uniform(1.0, 3.0, 3).round(3))
        res = tuple(int(r) for r in rng.integers(1, 70, 3))
        extend = tuple(rng.choice(S.ALL6, int(rng.integers(0, 7))))
        p = ns.Points(np.zeros((3, 0)))
        p._points = cloud
        got = p.to_image(size, res, extend)
        want = S.to_image_restated(cloud, size, res, extend)
        assert np.array_equal(got, want), (trial, size, res, extend)


def test_edge_sizes():
    p = ns.Points(np.zeros((3, 0)))
    p.move((1.0, 2.0, 3.0))
    assert p.cloud.shape == (3, 0)
    assert not p.to_image((2, 2, 2), (5, 5, 5), ()).any()
    one = ns.Points(np.zeros((3, 0)))
    one._points = np.asarray([[0.1], [0.2], [0.3]])          # (3, 1): Points() itself would transpose it to (1, 3)
    g = one.to_image((1, 1, 1), (11, 11, 11), ("-Z", "+X"))
    assert np.array_equal(g, S.to_image_restated(one.cloud, (1, 1, 1), (11, 11, 11), ("-Z", "+X")))
    dup = ns.Points(np.zeros((3, 0)))
    dup._points = np.tile(np.asarray([[0.25], [-0.25], [0.0]]), (1, 1000000))
    g = dup.to_image((1, 1, 1), (9, 9, 9), ())
    assert np.count_nonzero(g) == 1 and g[6, 2, 4] == 1.0


def test_grid_above_2_31_voxels():
    res = (2049, 1025, 1025)
    n = res[0] * res[1] * res[2]
    assert n > 2 ** 31
    # A = (1, 1, 1): the last voxel (2048, 1024, 1024), on the last edges; B = (0, 0, 0): (1024, 512, 512);
    # C = (-0.5, 1, 0): (512, 1024, 512). -X copies plane x = 512 (C alone) below it, then -Z copies plane z = 512.
    cloud = np.asarray([[1.0, 0.0, -0.5], [1.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    p = ns.Points(np.zeros((3, 0)))
    p._points = cloud
    dev = p.to_image_resident((2, 2, 2), res, ("-X", "-Z"))
    try:
        def voxel(i, j, k):
            v = np.empty(1, dtype=np.float32)
            off = ((i * res[1] + j) * res[2] + k) * 4
            _engine.check(_engine.lib().sdfk_memcpy_d2h(v.ctypes.data_as(ctypes.c_void_p),
                                                        ctypes.c_void_p(dev.ptr + off), 4), "sdfk_memcpy_d2h")
            return float(v[0])
        assert dev.n == n
        assert voxel(2048, 1024, 1024) == 1.0 and voxel(1024, 512, 512) == 1.0 and voxel(512, 1024, 512) == 1.0
        assert voxel(0, 1024, 512) == 1.0 and voxel(511, 1024, 512) == 1.0          # -X
        assert voxel(0, 1024, 0) == 1.0 and voxel(512, 1024, 0) == 1.0 and voxel(1024, 512, 0) == 1.0     # -Z
        assert voxel(2048, 1024, 0) == 0.0 and voxel(2048, 1024, 1023) == 0.0 and voxel(513, 1024, 0) == 0.0
        assert voxel(0, 0, 0) == 0.0 and voxel(1024, 512, 513) == 0.0 and voxel(2047, 1024, 1024) == 0.0
    finally:
        dev.free()


def test_deterministic():
    rng = np.random.default_rng(3)
    p = ns.Points(np.zeros((3, 0)))
    p._points = rng.normal(0, 0.5, (3, 200000))
    a = p.to_image((2, 2, 2), (65, 65, 65), ("-Z", "+Z", "-X"))
    b = p.to_image((2, 2, 2), (65, 65, 65), ("-Z", "+Z", "-X"))
    assert np.array_equal(a, b)


def _close(got, want, co=None, threshold=None, scale=1.0):
    """|got - want| <= 1e-6 max(1, |want|) (times `scale`: the edge stencil's weights add up to 16 in absolute value, so
    its result carries the fp32 rounding of operands up to 16 times its own size); with a threshold, points whose circle SDF lies within 1e-6 of it (exact ties
    of hard_binarization, where the fp32 field and the float64 reference fall on different sides) are exempt."""
    got = np.asarray(got, dtype=np.float64)
    if got.shape != want.shape:
        return False
    ok = np.abs(got - want) <= 1e-6 * scale * np.maximum(1.0, np.abs(want))
    if threshold is not None:
        sdf = np.hypot(co[0], co[1]) - 1.0
        ok |= (np.abs(sdf - threshold) <= 1e-6).reshape(ok.shape)
    return bool(ok.all())


def test_post_process_fields(golden):
    meta, arrays = golden
    co, _ = ns.generate_grid(S.PP_SIZE, S.PP_RES)
    co = S.f32(co)
    bad = []
    for label, method, args in S.pp_methods(S.PP_RES):
        got, pp = S.pp_field(ns, method, args, co)
        mod = ns.Circle(1)
        getattr(mod, method)(*args)
        want = mod.create(co)
        assert np.asarray(got).shape == np.asarray(want).shape and np.array_equal(got, want), label
        direct = pp.processed_geo_object(co)                   # the closure called directly, as in the reference
        assert np.array_equal(direct, got), label
        if not _close(got, arrays["pp_%s" % label], co, args[0] if method == "hard_binarization" else None,
                      16.0 if method == "conv_edge_detection" else 1.0):
            w = arrays["pp_%s" % label]
            bad.append((label, float(np.abs(np.asarray(got, dtype=np.float64) - w).max())))
    assert not bad, bad
    got, _ = S.pp_chain_field(ns, co)
    assert _close(got, arrays["pp_chain"])


def test_example_scripts(golden):
    meta, arrays = golden
    for path, (size, _res), builder, names in S.SCRIPTS:
        stem = os.path.splitext(os.path.basename(path))[0]
        co, _ = ns.generate_grid(size, S.SCRIPT_SMALL_RES)
        out = builder(ns, S.f32(co))
        for var, key in names.items():
            got = out if key is None else out[key]
            thr = 0 if var == "hb_geo_field" else None
            assert _close(got, arrays["script_%s_%s" % (stem, var)], S.f32(co), thr), (stem, var)
