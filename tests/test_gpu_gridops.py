"""GPU tests of csrc/sdfk_gridops.inc through the C-ABI (run with -m gpu on an MI355X): every variant of the box kernels
bit for bit against the plain reference of tests/gridops_reference.py on noise, sdfk_field_min, and the parts of `signed`
(caller scratch, the "already signed" return, the slab entry points) that tests/test_gpu_parity.py leaves out.

Every field and scratch buffer is followed by GUARD bytes of a fixed pattern which must be unchanged after the call:
a store past the end is a failed assertion here."""
import ctypes
import functools

import numpy as np
import pytest

import gridops_reference as gr
import aegolius_amd.cores as ns
from gridops_reference import CASES
from test_gpu_parity import _signed_numpy

pytestmark = pytest.mark.gpu

GUARD = 256
PATTERN = 0xA5


class Guarded:
    """`nbytes` of device memory at `offset` bytes past a 256-byte boundary, with GUARD pattern bytes behind them."""

    def __init__(self, engine, nbytes, offset=0):
        self.engine, self.lib, self.nbytes, self.offset = engine, engine.lib(), int(nbytes), offset
        self.base = self.lib.sdfk_malloc(offset + self.nbytes + GUARD)
        assert self.base and self.base % 256 == 0
        self.ptr = ctypes.c_void_p(self.base + offset)
        self.put(np.full(self.nbytes, PATTERN, dtype=np.uint8))

    def put(self, host):
        host = np.ascontiguousarray(host)
        assert host.nbytes == self.nbytes
        both = np.concatenate([host.view(np.uint8).ravel(), np.full(GUARD, PATTERN, dtype=np.uint8)])
        self.engine.check(self.lib.sdfk_memcpy_h2d(self.ptr, both.ctypes.data_as(ctypes.c_void_p), both.nbytes), "h2d")
        return self

    def get(self, dtype=np.float32):
        """the contents; asserts that the guard is intact"""
        both = np.empty(self.nbytes + GUARD, dtype=np.uint8)
        self.engine.check(self.lib.sdfk_sync(None), "sync")
        self.engine.check(self.lib.sdfk_memcpy_d2h(both.ctypes.data_as(ctypes.c_void_p), self.ptr, both.nbytes), "d2h")
        assert np.all(both[self.nbytes:] == PATTERN), "bytes behind the buffer were overwritten"
        return both[:self.nbytes].view(dtype).copy()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.sdfk_free(ctypes.c_void_p(self.base))


def _box(engine, host, ks, iterations=1, scratch=False):
    """sdfk_grid_box_average on a host array (2-D or 3-D), guards checked"""
    n, k = gr.dims3(host.shape), gr.dims3(ks)
    with Guarded(engine, host.nbytes) as field:
        field.put(host)
        tmp = Guarded(engine, host.nbytes) if scratch else None
        try:
            engine.check(engine.lib().sdfk_grid_box_average(field.ptr, n[0], n[1], n[2], k[0], k[1], k[2], iterations,
                                                            tmp.ptr if tmp else None, None), "sdfk_grid_box_average")
            if tmp:
                tmp.get()
        finally:
            if tmp:
                tmp.__exit__()
        return field.get().reshape(host.shape)


def _edge(engine, host, scratch=False):
    n = gr.dims3(host.shape)
    with Guarded(engine, host.nbytes) as field:
        field.put(host)
        tmp = Guarded(engine, host.nbytes) if scratch else None
        try:
            engine.check(engine.lib().sdfk_grid_edge_detect(field.ptr, n[0], n[1], n[2], tmp.ptr if tmp else None, None),
                         "sdfk_grid_edge_detect")
            if tmp:
                tmp.get()
        finally:
            if tmp:
                tmp.__exit__()
        return field.get().reshape(host.shape)


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    diff = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    if diff.size:
        at = np.unravel_index(diff[0], got.shape)
        raise AssertionError("%s: %d of %d points differ, first at %s: got %r, want %r"
                             % (what, diff.size, got.size, tuple(int(i) for i in at), got[at], want[at]))


def _variant(engine, shape, ks):
    out = (ctypes.c_int * 8)()
    n, k = gr.dims3(shape), gr.dims3(ks)
    engine.check(engine.lib().sdfk_debug_box_variant(n[0], n[1], n[2], k[0], k[1], k[2], out), "sdfk_debug_box_variant")
    return sorted(gr.variant_names(shape, ks, out))


@functools.lru_cache(maxsize=None)
def _dyadic_case(shape, ks):
    """(input, expected average): computed once, shared by the runs of a case, never written to"""
    rng = np.random.default_rng(sum(shape) * 31 + sum(ks))
    u = gr.dyadic(rng, shape)
    want = gr.box_average(u, ks)
    u.setflags(write=False)
    want.setflags(write=False)
    return u, want


_IDS = ["%s-%s" % ("x".join(map(str, s)), "x".join(map(str, k))) for s, k in CASES]


@pytest.mark.parametrize("no_march", [False, True], ids=["dispatched", "no_march"])
@pytest.mark.parametrize("shape,ks", CASES, ids=_IDS)
def test_box_average_bit_exact(shape, ks, no_march, engine, monkeypatch):
    """Every case of the list as the library dispatches it, and again with the marching kernel switched off, so that the
    tiled kernel also serves the shapes it normally never sees."""
    monkeypatch.delenv("SDFK_BOXM_SEG", raising=False)
    if no_march:
        monkeypatch.setenv("SDFK_BOX_NO_MARCH", "1")
    else:
        monkeypatch.delenv("SDFK_BOX_NO_MARCH", raising=False)
    u, want = _dyadic_case(shape, ks)
    _same_bits(_box(engine, u, ks), want, "%s kernel %s %s" % (shape, ks, _variant(engine, shape, ks)))


@pytest.mark.parametrize("seg", [1, 3])
@pytest.mark.parametrize("ks", [(3, 3, 3), (2, 4, 6), (7, 7, 7), (4, 2, 1), (5, 5, 5), (1, 1, 2)], ids=str)
def test_box_average_bit_exact_with_short_marching_segments(ks, seg, engine, monkeypatch):
    """segment seams on every plane (and every third): each workgroup starts from its own reflected halo planes"""
    monkeypatch.delenv("SDFK_BOX_NO_MARCH", raising=False)
    monkeypatch.setenv("SDFK_BOXM_SEG", str(seg))
    shape = (7, 9, 65)
    names = _variant(engine, shape, ks)
    assert "march: several segments" in names
    u, want = _dyadic_case(shape, ks)
    _same_bits(_box(engine, u, ks), want, "%s kernel %s segment %d %s" % (shape, ks, seg, names))


_EDGE_SHAPES = [(33, 9, 65), (5, 13, 130), (32, 8, 64), (1, 1, 1), (2, 2, 2), (1, 7, 3), (3, 1, 70), (70, 3, 1), (3, 2, 5),
                (1, 1, 4), (77, 130), (300, 2)]


@pytest.mark.parametrize("scratch", [False, True], ids=["null", "scratch"])
@pytest.mark.parametrize("shape", _EDGE_SHAPES, ids=str)
def test_edge_detection_bit_exact(shape, scratch, engine, monkeypatch):
    monkeypatch.delenv("SDFK_BOX_NO_MARCH", raising=False)
    monkeypatch.delenv("SDFK_BOXM_SEG", raising=False)
    u = gr.dyadic(np.random.default_rng(sum(shape)), shape)
    _same_bits(_edge(engine, u, scratch), gr.edge_detect(u), "edge filter on %s" % (shape,))


def test_edge_detection_bit_exact_on_the_tiled_kernel(engine, monkeypatch):
    monkeypatch.setenv("SDFK_BOX_NO_MARCH", "1")
    for shape in ((33, 9, 65), (77, 130), (3, 1, 70)):
        u = gr.dyadic(np.random.default_rng(sum(shape)), shape)
        _same_bits(_edge(engine, u), gr.edge_detect(u), "edge filter (tiled) on %s" % (shape,))


@pytest.mark.parametrize("scratch", [False, True], ids=["null", "scratch"])
@pytest.mark.parametrize("shape,ks", [((33, 9, 65), (3, 3, 3)), ((33, 9, 65), (9, 9, 9)), ((77, 130), (2, 4)), ((3, 2, 5), (9, 7, 13))],
                         ids=str)
def test_iterations_ping_pong(shape, ks, scratch, engine):
    """`iterations` passes in one call (field and scratch swap roles) = the same number of one-pass calls, bit for bit;
    none leaves the field's bits alone"""
    u = np.random.default_rng(5).normal(0.0, 1.0, shape).astype(np.float32)
    u.ravel()[3 % u.size] = np.float32(-0.0)
    _same_bits(_box(engine, u, ks, 0, scratch), u, "0 iterations")
    step = u
    for iterations in (1, 2, 3):
        step = _box(engine, step, ks, 1, scratch)
        _same_bits(_box(engine, u, ks, iterations, scratch), step, "%d iterations" % iterations)


def _inexact_fields(shape):
    rng = np.random.default_rng(11)
    # 1e-30 .. 1e30 within one field, the exponent running along the flat index so that the windows of every decade hold
    # values of their own size; and plain normal noise
    wide = rng.uniform(0.5, 1.0, shape) * rng.choice([-1.0, 1.0], shape) * 10.0 ** np.linspace(-30, 30, int(np.prod(shape))).reshape(shape)
    return {"1e-30..1e30": wide.astype(np.float32), "normal": rng.normal(0.0, 1.0, shape).astype(np.float32)}


@pytest.mark.parametrize("shape,ks", [((33, 9, 65), (3, 3, 3)), ((33, 9, 65), (2, 4, 6)), ((33, 9, 65), (9, 9, 9)), ((5, 13, 130), (6, 3, 3)),
                                      ((3, 2, 5), (9, 7, 13)), ((77, 130), (5, 5))], ids=str)
def test_box_average_on_inexact_inputs(shape, ks, engine):
    """|got - ref| <= 2^-24 |ref| + taps 2^-52 box_sum(|u|) / taps, ref the float64 average before its cast: the first
    term is the one fp32 rounding, the second the float64 roundings of the two summation orders — at most taps - 1 for
    the kernel's sum, k0 + k1 + k2 - 3 for the reference's axis-by-axis sum and one each for the scaling, of 2^-53 of the
    sum of magnitudes each, together no more than 2 taps 2^-53."""
    for name, u in _inexact_fields(shape).items():
        ref = gr.box_average64(u, ks)
        bound = 2.0 ** -24 * np.abs(ref) + gr.taps(ks) * 2.0 ** -52 * gr.box_sum(np.abs(u), ks) * (1.0 / gr.taps(ks))
        err = np.abs(_box(engine, u, ks).astype(np.float64) - ref)
        print("%s %s %s: max err / bound = %.3f" % (shape, ks, name, float(np.max(err / bound))))
        assert np.all(err <= bound), (name, float(np.max(err / bound)))


@pytest.mark.parametrize("shape", [(33, 9, 65), (5, 13, 130), (77, 130)], ids=str)
def test_edge_detection_on_inexact_inputs(shape, engine):
    """|got - ref| <= 2^-24 |ref| + 10 2^-52 (9 |u| + box_sum(|u|)): one fp32 rounding; in float64 the kernel rounds 8
    additions, the product and the difference, the reference 4 additions, the product and the difference — 16 roundings
    of 2^-53 (9 |u| + sum) at most, within 10 2^-52."""
    for name, u in _inexact_fields(shape).items():
        ref = gr.edge_detect64(u)
        mag = 9.0 * np.abs(u.astype(np.float64)) + gr.box_sum(np.abs(u), gr.edge_kernel(u.ndim))
        bound = 2.0 ** -24 * np.abs(ref) + 10 * 2.0 ** -52 * mag
        err = np.abs(_edge(engine, u).astype(np.float64) - ref)
        print("%s %s: max err / bound = %.3f" % (shape, name, float(np.max(err / bound))))
        assert np.all(err <= bound), (name, float(np.max(err / bound)))


@pytest.mark.parametrize("ks", [(3, 3, 3), (2, 4, 6), (9, 9, 9), (6, 3, 3), "edge"], ids=str)
def test_non_finite_values_stay_in_their_windows(ks, engine):
    """one NaN inside, +Inf and -Inf in opposite corners: the output is non-finite exactly where the reference's is and
    bit-equal elsewhere"""
    shape = (33, 9, 65)
    u = gr.dyadic(np.random.default_rng(2), shape).copy()
    u[16, 4, 30] = np.nan
    u[0, 0, 0] = np.inf
    u[32, 8, 64] = -np.inf
    with np.errstate(invalid="ignore"):
        want = gr.edge_detect(u) if ks == "edge" else gr.box_average(u, ks)
    got = _edge(engine, u) if ks == "edge" else _box(engine, u, ks)
    bad = ~np.isfinite(want)
    assert 3 <= bad.sum() < want.size // 2
    np.testing.assert_array_equal(~np.isfinite(got), bad)
    _same_bits(np.where(bad, np.float32(0), got), np.where(bad, np.float32(0), want), "finite part, kernel %s" % (ks,))


def test_python_surface_hands_the_shape_over(engine):
    """ns.conv_averaging / ns.conv_edge_detection on a 2-D and a 3-D array, the kernel as an int and as a tuple"""
    for shape, kernels in (((77, 130), (3, (3, 3), (2, 4), 6)), ((33, 9, 65), (3, (3, 3, 3), (2, 4, 6), (6, 3, 3)))):
        u = gr.dyadic(np.random.default_rng(len(shape)), shape)
        for kern in kernels:
            ks = (kern,) * len(shape) if isinstance(kern, int) else kern
            got = ns.conv_averaging(u.copy(), kern, 1)
            assert got.shape == shape
            _same_bits(got, gr.box_average(u, ks), "conv_averaging %s %r" % (shape, kern))
        _same_bits(ns.conv_averaging(u.copy(), kernels[1], 2), gr.box_average(gr.box_average(u, kernels[1]), kernels[1]),
                   "conv_averaging twice")
        _same_bits(ns.conv_edge_detection(u.copy()), gr.edge_detect(u), "conv_edge_detection %s" % (shape,))
    with pytest.raises(ValueError):
        ns.conv_averaging(np.zeros((4, 4, 4), dtype=np.float32), (3, 3), 1)


# ---- sdfk_field_min -------------------------------------------------------------------------------------------------
def _field_min(engine, host, offset=0):
    with Guarded(engine, host.nbytes, offset) as field:
        field.put(host)
        out = ctypes.c_float(7.0)
        rc = engine.lib().sdfk_field_min(field.ptr, host.size, ctypes.byref(out), None)
        _same_bits(field.get(), host, "sdfk_field_min reads only")
        return rc, np.float32(out.value)


_MIN_SIZES = (1, 2, 3, 4, 5, 1023, 1024, 1025, 2 ** 21 + 5)       # the last: more than 2048 workgroups cover in one stride


@pytest.mark.parametrize("n", _MIN_SIZES)
def test_field_min_finds_the_minimum_wherever_it_sits(n, engine):
    base = np.random.default_rng(n).uniform(0.5, 2.0, n).astype(np.float32)
    tail = n - n // 4 * 4
    spots = {0, min(3, n - 1), max(n // 4 * 4 - 4, 0), max(n // 4 * 4 - 1, 0), n // 2} | {n - 1 - t for t in range(tail)}
    for spot in sorted(spots):                                  # first quad, last quad, every element of the tail
        for value in (0.25, -3.0):
            host = base.copy()
            host[spot] = value
            rc, got = _field_min(engine, host)
            assert rc == 0 and got == np.min(host) == np.float32(value), (n, spot, got)
    rc, got = _field_min(engine, base)
    assert rc == 0 and got == np.min(base)


@pytest.mark.parametrize("n", [5, 1027])
def test_field_min_special_values(n, engine):
    rc, got = _field_min(engine, np.full(n, np.inf, dtype=np.float32))
    assert rc == 0 and got == np.inf
    for spot in (0, n - 1):                                     # a quad, the tail
        tiny = np.full(n, 1.0, dtype=np.float32)
        tiny[n // 2] = -np.float32(1e-45)
        tiny[spot] = -np.float32(3e-45)                         # negative denormals: ordered by their bits
        rc, got = _field_min(engine, tiny)
        assert rc == 0 and got == np.min(tiny) and got < 0 and got.view(np.uint32) == 0x80000002
        zeros = np.zeros(n, dtype=np.float32)
        zeros[spot] = -0.0
        rc, got = _field_min(engine, zeros)
        assert rc == 0 and got == 0 and not got < 0
        nan = np.random.default_rng(1).uniform(-1.0, 1.0, n).astype(np.float32)
        nan[spot] = np.nan
        rc, got = _field_min(engine, nan)
        assert rc == 0 and np.isnan(got)


def test_field_min_refuses_a_misaligned_field(engine):
    host = np.arange(9, dtype=np.float32)
    for offset in (4, 8, 12):
        rc, _ = _field_min(engine, host, offset)
        assert rc == -1 and "16-byte aligned" in engine.last_error()
    assert _field_min(engine, host, 16) == (0, np.float32(0.0))


# ---- signed: what test_signed_bit_planes_on_awkward_shapes leaves out ------------------------------------------------------
def _noise(shape, seed):
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.0, 1.0, shape)
    s[rng.uniform(size=shape) < 0.3] = 0.0                      # blobs as well as noise, as in the awkward-shapes test
    return np.ascontiguousarray(s, dtype=np.float32)


def _signed(engine, host, sep, crop, scratch=False, offset=0):
    with Guarded(engine, host.nbytes, offset) as field:
        field.put(host)
        tmp = Guarded(engine, host.nbytes) if scratch else None
        try:
            engine.check(engine.lib().sdfk_grid_signed(field.ptr, host.shape[0], host.shape[1], host.shape[2], float(np.float32(sep)),
                                                       crop, tmp.ptr if tmp else None, None), "sdfk_grid_signed")
            if tmp:
                tmp.get()
        finally:
            if tmp:
                tmp.__exit__()
        return field.get().reshape(host.shape)


def _signed_want(host, sep, crop):
    return _signed_numpy(host.astype(np.float64), np.float64(np.float32(sep)), bool(crop)).astype(np.float32)


# the work arrays (24 bytes per 32 points of a row, rounded up) fit 3 of the scratch's 4 bytes per point from about 9
# points per row on; include/sdfk.h promises it from 11
_SIGNED_SHAPES = [(6, 5, 5), (6, 5, 8), (6, 5, 9), (3, 40, 10), (5, 4, 11), (4, 6, 12), (7, 5, 33), (9, 7, 65)]


@pytest.mark.parametrize("crop", [1, 0])
@pytest.mark.parametrize("shape", _SIGNED_SHAPES, ids=str)
def test_signed_with_caller_scratch(shape, crop, engine):
    host = _noise(shape, sum(shape) + crop)
    want = _signed_want(host, 0.5, crop)
    assert (want < 0).any()
    _same_bits(_signed(engine, host, 0.5, crop, scratch=False), want, "signed, own scratch")
    _same_bits(_signed(engine, host, 0.5, crop, scratch=True), want, "signed, caller scratch")


@pytest.mark.parametrize("scratch", [False, True], ids=["null", "scratch"])
@pytest.mark.parametrize("shape", [(6, 5, 8), (9, 7, 65)], ids=str)
def test_signed_returns_an_already_signed_field_untouched(shape, scratch, engine):
    """one negative value, one negative denormal or one NaN anywhere: the field comes back bit for bit; -0.0 is no
    negative value"""
    base = _noise(shape, 3)
    assert (_signed_want(base, 0.5, 1) < 0).any()
    for spot in ((0, 0, 0), (shape[0] - 1, shape[1] - 1, shape[2] - 1), (shape[0] // 2, shape[1] // 2, shape[2] // 2)):
        for value in (np.float32(-0.75), -np.float32(1e-45), np.float32(np.nan)):
            host = base.copy()
            host[spot] = value
            _same_bits(_signed(engine, host, 0.5, 1, scratch), host, "signed of a field holding %r at %s" % (value, spot))
        host = base.copy()
        host[spot] = np.float32(-0.0)
        want = _signed_want(host, 0.5, 1)
        assert (want < 0).any()
        _same_bits(_signed(engine, host, 0.5, 1, scratch), want, "signed of a field holding -0.0 at %s" % (spot,))


@pytest.mark.parametrize("shape", [(6, 5, 8), (9, 7, 65), (7, 5, 33)], ids=str)
def test_signed_takes_any_float_alignment(shape, engine):
    host = _noise(shape, 9)
    for crop in (1, 0):
        _same_bits(_signed(engine, host, 0.5, crop, offset=4), _signed_want(host, 0.5, crop), "signed, field 4 bytes off")


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1027])
def test_boundary_mask(n, engine):
    host = np.random.default_rng(n).uniform(0.0, 1.0, max(n, 1)).astype(np.float32)[:n]
    sep = np.float32(0.4)
    if n:
        host[n // 2] = sep                                      # not below the threshold
    with Guarded(engine, n * 4) as field, Guarded(engine, n) as mask:
        field.put(host)
        engine.check(engine.lib().sdfk_grid_boundary_mask(field.ptr, n, float(sep), mask.ptr, None), "sdfk_grid_boundary_mask")
        np.testing.assert_array_equal(mask.get(np.uint8), (host < sep).astype(np.uint8))
        _same_bits(field.get(), host, "the field is only read")


@pytest.mark.parametrize("crop", [1, 0])
@pytest.mark.parametrize("shape", [(12, 9, 129), (17, 33, 31), (9, 7, 65)], ids=str)
def test_signed_slabs_put_together_equal_the_whole(shape, crop, engine):
    """uneven slabs of planes — one plane alone at either end, slabs that neither start at nor span a multiple of the 8
    planes a workgroup flips — on the whole grid's mask: bit for bit sdfk_grid_signed of the whole field"""
    lib = engine.lib()
    n0, n1, n2 = shape
    sep = np.float32(0.5)
    host = _noise(shape, sum(shape) + 7 * crop)
    whole = _signed(engine, host, sep, crop)
    _same_bits(whole, _signed_want(host, sep, crop), "signed, whole field")
    assert (whole < 0).any()
    cuts = [0, 1, 4, n0 - 1, n0]
    with Guarded(engine, host.nbytes) as field, Guarded(engine, host.size) as mask:
        field.put(host)
        engine.check(lib.sdfk_grid_boundary_mask(field.ptr, host.size, float(sep), mask.ptr, None), "sdfk_grid_boundary_mask")
        np.testing.assert_array_equal(mask.get(np.uint8), (host < sep).astype(np.uint8).ravel())
        parts = []
        for number, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            with Guarded(engine, host[a:b].nbytes) as slab:
                slab.put(host[a:b])
                tmp = Guarded(engine, host.nbytes) if number % 2 else None
                try:
                    engine.check(lib.sdfk_grid_signed_slab(slab.ptr, a, b - a, mask.ptr, n0, n1, n2, crop, tmp.ptr if tmp else None,
                                                           None), "sdfk_grid_signed_slab")
                    if tmp:
                        tmp.get()
                finally:
                    if tmp:
                        tmp.__exit__()
                parts.append(slab.get().reshape(b - a, n1, n2))
        mask.get(np.uint8)
    _same_bits(np.concatenate(parts), whole, "slabs %s of %s" % (cuts, shape))
