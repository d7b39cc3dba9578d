"""CPU (no GPU needed): the plain reference of the box kernels (tests/gridops_reference.py) equals scipy bit for bit on
exact inputs, and its case list reaches every variant the box dispatch of csrc/sdfk_gridops.inc has — asked of the
library itself (sdfk_debug_box_variant: host only, the launch reads the same decision)."""
import ctypes

import numpy as np
import pytest

import gridops_reference as gr
from gridops_reference import CASES

_SMALL = [(s, k) for s, k in CASES if s != gr.BIG] + [((12, 20, 9), (6, 3, 3))]


@pytest.mark.parametrize("shape,ks", _SMALL, ids=lambda v: "x".join(str(i) for i in v))
def test_reference_equals_scipy_bit_for_bit(shape, ks):
    """odd, even, mixed and wider-than-the-field kernels, 2-D and 3-D: box sum, average and the edge filter"""
    ndimage = pytest.importorskip("scipy.ndimage")
    from oracle import sdf_oracle
    rng = np.random.default_rng(sum(shape) * 31 + sum(ks))
    u32 = gr.dyadic(rng, shape)
    assert u32.dtype == np.float32 and np.all(u32.astype(np.float64) * 2.0 ** 12 == np.round(u32.astype(np.float64) * 2.0 ** 12))
    u = u32.astype(np.float64)
    ones = np.ones(ks)
    np.testing.assert_array_equal(gr.box_sum(u, ks), ndimage.convolve(u, ones))
    np.testing.assert_array_equal(gr.box_average(u, ks), (ndimage.convolve(u, ones) * (1.0 / gr.taps(ks))).astype(np.float32))
    # the oracle divides the filter before it sums: taps roundings of the products and of the sum
    oracle = sdf_oracle._conv_averaging(u, ks, 1)
    bound = gr.taps(ks) * 2.0 ** -52 * gr.box_sum(np.abs(u), ks) / gr.taps(ks)
    assert np.all(np.abs(oracle - gr.box_average64(u, ks)) <= bound)
    f = np.asarray([[-1, -1, -1], [-1, 8, -1], [-1, -1, -1]], dtype=np.float64)       # oracle/sdf_oracle._conv_edge_detection
    f = f if u.ndim == 2 else f[:, :, None]
    np.testing.assert_array_equal(gr.edge_detect64(u), ndimage.convolve(u, f))
    np.testing.assert_array_equal(gr.edge_detect(u), ndimage.convolve(u, f).astype(np.float32))


def test_reference_reflects_repeatedly_and_keeps_windows():
    """a kernel several times wider than the field (pad > 2n), hand-checked; a non-finite value reaches
    exactly the outputs whose window (offsets -((k-1)//2) .. k//2) holds it"""
    u = np.asarray([1.0, 2.0, 4.0])
    # offsets -4 .. 5 of (.. 2 1 | 1 2 4 | 4 2 1 | 1 2 4 ..): index -4 .. 7 = 4 4 2 1 | 1 2 4 | 4 2 1 1 2
    ext = np.asarray([4, 4, 2, 1, 1, 2, 4, 4, 2, 1, 1, 2], dtype=np.float64)
    np.testing.assert_array_equal(gr.box_sum(u, (10,)), [ext[i:i + 10].sum() for i in range(3)])
    v = np.zeros((5, 5))
    v[2, 2] = np.inf
    assert np.array_equal(~np.isfinite(gr.box_sum(v, (3, 2))), np.isin(np.arange(5), (1, 2, 3))[:, None] & np.isin(np.arange(5), (1, 2))[None, :])


def _variant(built, shape, ks):
    out = (ctypes.c_int * 8)()
    n, k = gr.dims3(shape), gr.dims3(ks)
    built.check(built.lib().sdfk_debug_box_variant(n[0], n[1], n[2], k[0], k[1], k[2], out), "sdfk_debug_box_variant")
    return list(out)


def test_cases_reach_every_box_variant(built, monkeypatch):
    monkeypatch.delenv("SDFK_BOX_NO_MARCH", raising=False)
    monkeypatch.delenv("SDFK_BOXM_SEG", raising=False)
    reached = set()
    for shape, ks in CASES:
        reached |= gr.variant_names(shape, ks, _variant(built, shape, ks))
    assert not (gr.ALL_VARIANTS - reached), "no case reaches: %s" % sorted(gr.ALL_VARIANTS - reached)
    assert not (reached - gr.ALL_VARIANTS), sorted(reached - gr.ALL_VARIANTS)


def test_box_variant_query(built, monkeypatch):
    """the query's record on a few launches worked out by hand, the two overrides, and its argument checks"""
    monkeypatch.delenv("SDFK_BOX_NO_MARCH", raising=False)
    monkeypatch.delenv("SDFK_BOXM_SEG", raising=False)
    MARCH, FAST, FLAT = 1, 2, 4
    # marching: 8 rows x 64 columns x 32 planes per workgroup
    assert _variant(built, (33, 9, 65), (3, 3, 3)) == [MARCH | FAST, 3, 3, 32, 1, 2, 2, 2]
    assert _variant(built, (33, 9, 65), (2, 4, 6)) == [MARCH | FAST, 2, 0, 32, 1, 2, 2, 2]
    # tiled: 4 rows per workgroup, one launch slot per plane; (4 + 8) * (64 + 8) = 864 cells -> 8 planes per chunk
    assert _variant(built, (33, 9, 65), (9, 9, 9)) == [FAST, 0, 0, 8, 2, 2, 3, 33]
    assert _variant(built, (33, 9, 65), (6, 3, 3)) == [FAST, 0, 3, 6, 1, 2, 3, 33]
    assert _variant(built, (33, 9, 65), (3, 8, 7)) == [FAST, 0, 7, 3, 1, 2, 3, 33]          # 15 * 70 > 1024
    assert _variant(built, (3, 2, 5), (9, 7, 13)) == [0, 0, 0, 9, 1, 1, 1, 3]
    assert _variant(built, (128, 512, 65), (6, 3, 3)) == [FAST, 0, 3, 6, 1, 1, 128, 128]    # 16384 rows: gx = 1 of 2 k tiles
    assert _variant(built, (77, 130), (3, 3)) == [MARCH | FAST | FLAT, 1, 3, 32, 1, 3, 10, 1]
    assert _variant(built, (70, 3, 1), (2, 4, 2)) == [MARCH | FAST | FLAT, 1, 0, 32, 1, 1, 9, 1]   # k2 folded away
    monkeypatch.setenv("SDFK_BOXM_SEG", "3")
    assert _variant(built, (7, 9, 65), (3, 3, 3)) == [MARCH | FAST, 3, 3, 3, 1, 2, 2, 3]
    monkeypatch.setenv("SDFK_BOX_NO_MARCH", "1")
    assert _variant(built, (7, 9, 65), (3, 3, 3)) == [FAST, 0, 3, 3, 1, 2, 3, 7]
    out = (ctypes.c_int * 8)()
    lib = built.lib()
    assert lib.sdfk_debug_box_variant(0, 1, 1, 1, 1, 1, out) == -1
    assert lib.sdfk_debug_box_variant(4, 4, 4, 1, 0, 1, out) == -1
    assert lib.sdfk_debug_box_variant(4, 4, 4, 1, 1, 1, None) == -1
    assert lib.sdfk_debug_box_variant(4, 4, 4, 1, 200, 200, out) == -1 and "too wide" in built.last_error()
