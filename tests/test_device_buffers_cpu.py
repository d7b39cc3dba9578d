"""_engine.DeviceBuffer / DeviceRows and the functions built on them, without a GPU: a stand-in takes the place of the
library's device plumbing (host memory behind sdfk_malloc / sdfk_free / sdfk_memcpy_*, host-only entry points forwarded
to the built library, kernel launches answered with 0) and keeps the set of live allocations. Round trips, ownership,
and failure injection: whichever allocation or upload fails, a front end raises SdfkError and leaves nothing allocated."""
import collections
import ctypes
import gc
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import aegolius_amd.cores as ns  # noqa: E402
import scenes as S  # noqa: E402
from aegolius_amd import _eval, _points, autodiff, mesh  # noqa: E402
from aegolius_amd._lower import lower_geometry  # noqa: E402

SIZES = (0, 1, 63, 64, 65)


def _addr(p):
    return (p.value if isinstance(p, ctypes.c_void_p) else p) or 0


class FakeDevice:
    """Stands for libsdfk.so: "device" memory is host memory, nothing is launched."""
    HOST_ONLY = ("sdfk_last_error", "sdfk_linspace_f32", "sdfk_point_tree_build", "sdfk_dual_has_rule", "sdfk_vjp_limits")

    def __init__(self, real):
        self.real = real
        self.live, self.freed, self.bad_frees = {}, [], []
        self.calls = collections.Counter()
        self.mallocs, self.fail_malloc_at, self.fail_h2d = 0, None, False
        self.count = 0                       # what every counting entry point reports (selected points, vertices, faces)

    def sdfk_device_count(self):
        return 1

    def sdfk_malloc(self, nbytes):
        self.mallocs += 1
        if self.mallocs == self.fail_malloc_at:
            return None
        buf = ctypes.create_string_buffer(max(int(nbytes), 1))
        self.live[ctypes.addressof(buf)] = buf
        return ctypes.addressof(buf)

    def sdfk_free(self, p):
        if self.live.pop(_addr(p), None) is None:
            self.bad_frees.append(_addr(p))
        self.freed.append(_addr(p))
        return 0

    def _inside(self, p, nbytes):
        a = _addr(p)
        assert any(base <= a and a + nbytes <= base + len(buf) for base, buf in self.live.items()), "copy outside a live buffer"
        return a

    def sdfk_memcpy_h2d(self, dst, src, nbytes):
        if self.fail_h2d:
            self.fail_h2d = False
            return -5
        ctypes.memmove(self._inside(dst, nbytes), _addr(src), nbytes)
        return 0

    def sdfk_memcpy_d2h(self, dst, src, nbytes):
        ctypes.memmove(_addr(dst), self._inside(src, nbytes), nbytes)
        return 0

    def sdfk_memcpy_d2d(self, dst, src, nbytes):
        ctypes.memmove(self._inside(dst, nbytes), self._inside(src, nbytes), nbytes)
        return 0

    def __getattr__(self, name):
        if not name.startswith("sdfk_"):
            raise AttributeError(name)
        if name.startswith("sdfk_program_") or name.endswith("_scratch") or name in self.HOST_ONLY:
            return getattr(self.real, name)

        def launch(*args):
            self.calls[name] += 1
            for a in args:                   # byref(c_int64) arguments are counts the entry point reports
                obj = getattr(a, "_obj", None)
                if isinstance(obj, ctypes.c_int64):
                    obj.value = self.count
            return 0
        return launch


@pytest.fixture
def fake(built):
    real = built.lib()
    dev = FakeDevice(real)
    built._lib = dev
    try:
        yield dev
    finally:
        built._lib = real


def _clean(dev):
    """Nothing is allocated, and nothing was freed twice (a second free finds its pointer no longer live)."""
    gc.collect()
    return not dev.live and not dev.bad_frees


# ---- round trips ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_round_trips(built, fake, n):
    rng = np.random.default_rng(n)
    data = rng.standard_normal(n).astype(np.float32)
    with built.DeviceBuffer(4 * n + 8, what="test") as buf:
        assert buf.nbytes == 4 * n + 8 and isinstance(buf.ptr, int)
        buf.upload(data, 8)
        assert np.array_equal(buf.download(np.empty(n, dtype=np.float32), 8), data)
    rows = rng.standard_normal((3, n)).astype(np.float32)
    with built.DeviceRows(3, n) as d:
        assert d.stride == built.row_stride(n) == (n + 63) // 64 * 64 and d.stride % 64 == 0 and d.stride >= n
        for r in range(3):
            assert d.row_ptr(r) == d.ptr + 4 * r * built.row_stride(n) and d.row(r).value == d.row_ptr(r)
        d.upload_rows(rows)
        assert np.array_equal(d.download_rows(), rows)
        assert np.array_equal(d.download_rows(2), rows[:2])
        with built.DeviceBuffer(4 * n) as copy:
            copy.copy_from(d.row_ptr(1), 4 * n)
            assert np.array_equal(copy.download(np.empty(n, dtype=np.float32)), rows[1])
    f = built.DeviceField.from_host(data)
    assert (f.n, f.device, f.nbytes) == (n, 0, 4 * n) and np.array_equal(f.numpy(), data)
    v = built.DeviceVectorField.from_host(rows)
    assert (v.n, v.shape, v.stride) == (n, (3, n), built.row_stride(n)) and np.array_equal(v.numpy(), rows)
    with built.DeviceCoords(v) as borrowed, built.DeviceCoords(rows.astype(np.float64)) as owned:
        assert (borrowed.ptr, borrowed.stride, borrowed.n) == (v.row_ptr(0), v.stride, n) and borrowed.owned is None
        assert np.array_equal(owned.owned.download_rows(), rows) and (owned.stride, owned.n) == (v.stride, n)
    assert len(fake.live) == 2                                     # the borrowed field is still its owner's
    f.free()
    v.free()
    assert _clean(fake)


def test_argument_helpers(built):
    with pytest.raises(ValueError, match=r"coordinates must have shape \(3, N\); got \(2, 5\)"):
        built.host_coords(np.zeros((2, 5)))
    with pytest.raises(ValueError, match=r"coordinates must have shape \(3, N\)"):
        autodiff._point_count(np.zeros(7))
    assert autodiff._point_count(np.zeros((3, 7))) == 7
    assert built.host_coords(np.zeros((3, 2), np.float32)).dtype == np.float32
    assert built.host_coords(np.zeros((3, 2), np.float64)).dtype == np.float64
    assert built.host_coords(np.zeros((3, 2), np.int32)).dtype == np.float64
    assert built.host_coords(np.zeros((3, 2), np.float64), np.float32).dtype == np.float32
    assert built.host_coords(np.zeros((4, 3)).T).flags.c_contiguous
    axes = [np.linspace(0, 1, 4), np.arange(3, dtype=np.float32), np.zeros(1)]
    tables, args = built.axis_args(axes)
    assert [t.dtype for t in tables] == [np.float32] * 3 and all(t.flags.c_contiguous for t in tables)
    assert [a for a in args[1::2]] == [4, 3, 1]
    assert [p.value for p in args[0::2]] == [t.ctypes.data for t in tables]
    assert tables[1] is axes[1]                                    # already a float32 table: not copied


# ---- ownership --------------------------------------------------------------------------------------------------------------
def test_ownership(built, fake):
    buf = built.DeviceBuffer(16, what="scratch")
    p = buf.ptr
    buf.free()
    buf.free()                                                     # idempotent
    assert buf.ptr is None and fake.freed == [p]
    with pytest.raises(built.SdfkError, match="scratch has been freed"):
        buf.at()
    with pytest.raises(built.SdfkError, match="has been freed"):
        buf.upload(np.zeros(1, np.float32))
    with built.DeviceBuffer(16) as inside:
        assert inside.ptr in fake.live
    assert inside.ptr is None
    with pytest.raises(KeyError):
        with built.DeviceRows(2, 5) as rows:
            raise KeyError("x")
    assert rows.ptr is None
    built.DeviceBuffer(32)                                         # never bound: collected at once
    kept = built.DeviceField(5)
    del kept
    assert _clean(fake) and len(fake.freed) == 5

    f, v = built.DeviceField.from_host(np.ones(4, np.float32)), built.DeviceVectorField.from_host(np.ones((3, 4), np.float32))
    f.free()
    v.free()
    assert f.ptr is None and v.ptr is None
    for use in (f.numpy, f._live, f.select, f.count, v.numpy, lambda: v.row_ptr(0)):
        with pytest.raises(built.SdfkError, match="Device(Vector)?Field has been freed"):
            use()
    assert _clean(fake)


def test_bounds_are_checked_before_the_library(built, fake):
    with built.DeviceBuffer(16) as buf:
        assert buf.at(16).value == buf.ptr + 16
        for args in ((17,), (-1,), (8, 9), (0, -1)):
            with pytest.raises(built.SdfkError, match="outside"):
                buf.at(*args)
        with pytest.raises(built.SdfkError, match="outside"):
            buf.upload(np.zeros(5, np.float32))
        with pytest.raises(built.SdfkError, match="outside"):
            buf.upload(np.zeros(4, np.float32), 4)
        with pytest.raises(built.SdfkError, match="outside"):
            buf.download(np.zeros(5, np.float32))
        with pytest.raises(built.SdfkError, match="outside"):
            buf.copy_from(buf.ptr, 17)
        with pytest.raises(ValueError, match="contiguous"):
            buf.download(np.zeros((2, 4), np.float32)[:, :2])
    with built.DeviceRows(2, 3) as rows:
        with pytest.raises(built.SdfkError, match="outside"):
            rows.row(2)
    assert not any(fake.calls[c] for c in ("sdfk_memcpy_h2d", "sdfk_memcpy_d2h", "sdfk_memcpy_d2d")) and _clean(fake)


def test_out_of_memory_message(built, fake):
    fake.fail_malloc_at = 1
    with pytest.raises(built.SdfkError, match=r"^tangents: out of device memory \(12 bytes\): "):
        built.DeviceBuffer(12, what="tangents")
    fake.fail_malloc_at = 2
    with pytest.raises(built.SdfkError, match=r"^DeviceField: out of device memory \(20 bytes\): "):
        built.DeviceField(5)
    assert _clean(fake)


def test_no_events_without_timings(built, fake):
    tables = [np.linspace(-1, 1, 5, dtype=np.float32)] * 3
    mesh._extract(np.zeros(125, np.float32), tables, 0.0)
    _points.to_image(np.zeros((3, 4)), (2, 2, 2), (4, 4, 4), ())
    assert fake.calls["sdfk_event_create"] == 0 and fake.calls["sdfk_event_record"] == 0
    timer = built.Timer(None)
    timer.mark("a")
    timer.finish()
    assert timer.events == [] and _clean(fake)


# ---- failure injection --------------------------------------------------------------------------------------------------------
def _staged():
    build, key = S.GRID_SCENES["grid_conv_sphere_3x3x3"]
    co, res = S.grid_inputs(ns, key)
    return lambda: build(ns, res).create(co)


def _apply_fields():
    u = np.linspace(-1, 1, 70).reshape(7, 10)
    return lambda: _eval.apply_value_op("relu", u, {"width": 1})


def _grad_points():
    co = np.random.default_rng(3).uniform(-1, 1, (3, 70))
    return lambda: autodiff.value_and_grad_points(ns.Sphere(0.5), co)


def _select_host():
    co = np.random.default_rng(4).uniform(-1, 1, (3, 70))
    return lambda: _eval.program_for(lower_geometry(ns.Sphere(0.5))).select_host(co)


def _mesh_extract():
    tables = [np.linspace(-1, 1, 5, dtype=np.float32)] * 3
    return lambda: mesh._extract(np.zeros(125, np.float32), tables, 0.0)


def _to_image():
    cloud = np.random.default_rng(5).uniform(-1, 1, (3, 20))
    return lambda: _points.to_image(cloud, (2, 2, 2), (4, 4, 4), (), transfer="f64")


# (function under test, allocations one call makes)
FRONT_ENDS = {"_eval._run_staged": (_staged, 3), "_eval.apply_fields": (_apply_fields, 2), "autodiff._run": (_grad_points, 7),
              "Program.select_host": (_select_host, 3), "mesh._extract": (_mesh_extract, 4), "_points.to_image": (_to_image, 4)}


@pytest.mark.parametrize("name", sorted(FRONT_ENDS))
def test_a_failing_allocation_or_upload_leaves_nothing_allocated(built, fake, name):
    make, expected = FRONT_ENDS[name]
    call = make()
    fake.count = 3                                                 # selections and meshes are not empty: every buffer is made
    call()
    allocations = fake.mallocs
    assert allocations == expected and _clean(fake)
    for k in range(1, allocations + 1):
        fake.mallocs, fake.fail_malloc_at = 0, k
        with pytest.raises(built.SdfkError, match="out of device memory"):
            call()
        assert not fake.live and not fake.bad_frees, (name, k, len(fake.live))
    fake.mallocs, fake.fail_malloc_at, fake.fail_h2d = 0, None, True
    with pytest.raises(built.SdfkError, match=r"sdfk_memcpy_h2d failed \(-5\)"):
        call()
    assert not fake.live and not fake.bad_frees, (name, "h2d")
    assert _clean(fake)
