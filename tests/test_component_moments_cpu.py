"""CPU (no GPU needed): the numpy reference of the component moments (tests/component_moments_reference.py) against a
per-component Python loop, and the host arithmetic of aegolius_amd.topology.ComponentMoments — index moments, mass
properties of blocks of cells in closed form, totals, non-uniform tables, the wrap bound, dropped labels."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import component_moments_reference as CM  # noqa: E402
import topology_reference as R  # noqa: E402
from aegolius_amd import topology  # noqa: E402
from aegolius_amd.moments import MassProperties  # noqa: E402

SHAPES = ((7, 9), (2, 2), (5, 4, 6), (3, 5, 7), (2, 2, 2))


def _loop_sums(labels, count):
    """Per component, per point: Python ints."""
    d = labels.ndim
    rows = []
    for k in range(count):
        pts = [tuple(int(i) for i in p) for p in np.argwhere(labels == k)]
        row = [len(pts)] + [sum(p[a] for p in pts) for a in range(d)]
        row += [sum(p[a] * p[b] for p in pts) for a, b in CM.PAIRS[d]]
        rows.append(row)
    return rows


def _random_labellings():
    rng = np.random.default_rng(77)
    for shape in SHAPES:
        for density in (0.3, 0.6, 1.0):
            for connectivity in ("faces", "full"):
                yield R.label(rng.random(shape) < density, connectivity)


def test_reference_equals_a_python_loop():
    seen = 0
    for c in _random_labellings():
        got = CM.sums(c.labels, c.count)
        assert got.dtype == np.uint64 and got.shape == (c.count, 10 if c.labels.ndim == 3 else 6)
        assert [[int(v) for v in row] for row in got] == _loop_sums(c.labels, c.count)
        np.testing.assert_array_equal(got[:, 0], c.sizes.astype(np.uint64))
        seen += c.count
    assert seen > 50
    empty = CM.sums(np.full((3, 4), -1, dtype=np.int32), 0)
    assert empty.shape == (0, 6) and empty.dtype == np.uint64


def _tables(shape, lo=-1.0, hi=1.0):
    return [np.linspace(lo, hi, s) for s in shape]


def test_index_moments_are_sums_of_odd_lattice_coordinates():
    for c in _random_labellings():
        d = c.labels.ndim
        m = topology.ComponentMoments(CM.sums(c.labels, c.count), _tables(c.labels.shape))
        assert (m.count, m.dims, m.shape) == (c.count, d, c.labels.shape)
        for k in range(c.count):
            u = [[2 * int(i) + 1 for i in p] for p in np.argwhere(c.labels == k)]
            want = [len(u)] + [sum(p[a] for p in u) for a in range(d)] + [sum(p[a] * p[b] for p in u) for a, b in CM.PAIRS[d]]
            got = m.index_moments(k)
            assert got == tuple(want) and all(type(v) is int for v in got)


BLOCKS = (
    # shape, table ends, the block's index box (both ends included), density
    ((12, 9, 10), (-1.0, 1.0), ((2, 7), (1, 4), (3, 9)), 2.5),
    ((6, 5, 4), (999.0, 1001.0), ((0, 5), (0, 4), (0, 3)), 1.0),           # far from the origin: no cancellation
    ((20, 17), (-2.0, 3.0), ((4, 11), (0, 16)), 7850.0),
    ((5, 5, 5), (-1.0, 1.0), ((2, 2), (3, 3), (1, 1)), 1.0),               # one cell
)


@pytest.mark.parametrize("shape,ends,box,density", BLOCKS)
def test_properties_of_a_block_of_cells_are_closed_form(shape, ends, box, density):
    d = len(shape)
    tables = _tables(shape, *ends)
    labels = np.full(shape, -1, dtype=np.int32)
    k = 0 if all(lo == 0 for lo, _hi in box) else 1                         # (a block off the first point is the second
    labels[(0,) * d] = 0                                                    #  component: the first point is one of its own)
    labels[tuple(slice(lo, hi + 1) for lo, hi in box)] = k
    m = topology.ComponentMoments(CM.sums(labels, k + 1), tables, level=0.25)
    mp = m.properties(k, density)
    assert isinstance(mp, MassProperties) and mp.samples == 1 and mp.level == 0.25 and mp.near_cells == 0
    assert mp.index_moments == m.index_moments(k) and mp.shape == shape
    h = np.array([(t[-1] - t[0]) / (t.size - 1) for t in tables])
    lo = np.array([t[0] + (b[0] - 0.5) * s for t, b, s in zip(tables, box, h)])     # faces on cell boundaries
    hi = np.array([t[0] + (b[1] + 0.5) * s for t, b, s in zip(tables, box, h)])
    edge = hi - lo
    volume = float(np.prod(edge))
    mass = density * volume
    rel = 1e-12
    assert mp.volume == pytest.approx(volume, rel=rel) and mp.mass == pytest.approx(mass, rel=rel)
    np.testing.assert_allclose(mp.centroid, (lo + hi) / 2, rtol=rel, atol=rel * float(np.abs(edge).max()))
    second = mass * edge ** 2 / 12.0
    np.testing.assert_allclose(np.diag(mp.second_moments), second, rtol=rel)
    off = mp.second_moments - np.diag(np.diag(mp.second_moments))
    assert np.abs(off).max() <= rel * second.max()
    if d == 3:
        np.testing.assert_allclose(np.diag(mp.inertia), second.sum() - second, rtol=rel)
    else:
        assert mp.polar == pytest.approx(second.sum(), rel=rel)
    np.testing.assert_allclose(m.volumes[k], volume, rtol=rel)
    np.testing.assert_allclose(m.centroids[k], (lo + hi) / 2, rtol=rel, atol=rel * float(np.abs(edge).max()))


def test_total_is_the_sum_of_the_rows():
    for c in _random_labellings():
        sums = CM.sums(c.labels, c.count)
        m = topology.ComponentMoments(sums, _tables(c.labels.shape))
        width = sums.shape[1]
        want = tuple(sum(int(v) for v in sums[:, t]) for t in range(width))
        assert m.total() == want and all(type(v) is int for v in m.total())
        if c.count >= 2:
            some = np.zeros(c.count, dtype=bool)
            some[::2] = True
            by_ids = m.total(keep=np.flatnonzero(some))
            assert by_ids == m.total(keep=some) == tuple(sum(int(v) for v in sums[some][:, t]) for t in range(width))
            assert m.select(some).count == int(some.sum()) and m.select(some).total() == by_ids
            # the whole region as one solid: the index moments of the union are those of the mask
            on = c.labels >= 0
            one = topology.ComponentMoments(CM.sums(np.where(on, 0, -1), 1), _tables(c.labels.shape))
            assert topology.index_moments(m.total()) == one.index_moments(0)
            assert m.total_properties().index_moments == one.index_moments(0)
        with pytest.raises(ValueError, match="ids are"):
            m.total(keep=[c.count])
        with pytest.raises(ValueError, match="one entry per component"):
            m.total(keep=np.ones(c.count + 1, dtype=bool))
    huge = np.full((3, 6), 2 ** 63, dtype=np.uint64)                        # beyond uint64 when added: Python ints
    assert topology.ComponentMoments(huge, _tables((4, 4))).total() == (3 * 2 ** 63,) * 6


def test_non_uniform_tables_have_sums_but_no_world_quantities():
    tables = [np.array([0.0, 0.1, 0.5, 0.6, 2.0]), np.linspace(0, 1, 4)]
    c = R.label(np.random.default_rng(5).random((5, 4)) < 0.6, "faces")
    m = topology.ComponentMoments(CM.sums(c.labels, c.count), tables)
    assert m.sums.shape == (c.count, 6) and m.index_moments(0)[0] == int(c.sizes[0]) and m.total()[0] == int(c.sizes.sum())
    for call in (lambda: m.volumes, lambda: m.centroids, lambda: m.properties(0), lambda: m.total_properties()):
        with pytest.raises(ValueError, match="not uniform"):
            call()
    with pytest.raises(ValueError, match=r"shape \(K, 6\)"):
        topology.ComponentMoments(np.zeros((2, 10), dtype=np.uint64), tables)
    with pytest.raises(ValueError, match="integer array"):
        topology.ComponentMoments(np.zeros((2, 6)), tables)


def _refused(shape):
    n = math.prod(int(s) for s in shape)
    return any(n * (a - 1) * (b - 1) >= 2 ** 63 for a in shape for b in shape)


def test_wrap_bound_is_a_function_of_the_shape():
    assert not topology.sums_can_wrap((2, 1_000_000)) and not _refused((2, 1_000_000))
    assert topology.sums_can_wrap((65537, 32768)) and _refused((65537, 32768))
    assert 65537 * 32768 == 2 ** 31 + 32768 > topology.MAX_POINTS          # (label itself refuses that grid)
    d1 = 2_100_000                                                         # 2 d1 (d1 - 1)^2 = 1.85e19 >= 2^63 = 9.22e18
    assert 2 * d1 < topology.MAX_POINTS // 500 and 2 * d1 * (d1 - 1) ** 2 >= 2 ** 63
    assert topology.sums_can_wrap((2, d1)) and _refused((2, d1))
    edge = next(d for d in range(1_600_000, d1) if 2 * d * (d - 1) ** 2 >= 2 ** 63)     # the first refused length
    assert topology.sums_can_wrap((2, edge)) and not topology.sums_can_wrap((2, edge - 1))
    assert topology.sums_can_wrap((edge, 2)) and topology.sums_can_wrap((2, 3, edge))
    for shape in ((1290, 1290, 1290), (513, 513, 513), (2, 2), (46340, 46340)):
        assert topology.sums_can_wrap(shape) == _refused(shape)
    assert not topology.sums_can_wrap((1290, 1290, 1290))                   # the practical limit of `label` is far inside
    # refused by argument, before any device work: the message names the grid
    big = np.arange(d1, dtype=np.float32)
    with pytest.raises(ValueError, match="2x2100000"):
        topology.label(np.ones(2 * d1, dtype=np.float32), (np.arange(2, dtype=np.float32), big), moments=True)


def test_library_declares_the_entry_and_refuses_by_argument(built):
    header = open(os.path.join(os.path.dirname(HERE), "include", "sdfk.h")).read()
    assert "int sdfk_label_moments(" in header and "sdfk_label_moments" in built.SIGNATURES
    call = built.lib().sdfk_label_moments
    labels = built.ctypes.c_void_p(1 << 20)                    # (refused, or done, before the labels are looked at)
    assert call(2, 2_100_000, 1, labels, 1, labels, None, None) == -2
    assert "wrap" in built.last_error() and "2x2100000" in built.last_error()
    assert call(2, 1_000_000, 1, labels, 0, None, None, None) == 0          # no component: nothing to do
    assert call(2, 1_000_000, 1, None, 0, None, None, None) == -1
    assert call(2, 1_000_000, 1, built.ctypes.c_void_p((1 << 20) + 4), 1, labels, None, None) == -1
    assert "16-byte aligned" in built.last_error()
    assert call(1291, 1291, 1291, labels, 1, labels, None, None) == -1 and "2^31 - 1" in built.last_error()


def test_dropped_labels_raise():
    records = (np.zeros(1, dtype=np.int64), np.ones(1, dtype=np.int64), np.zeros((1, 2), dtype=np.int32),
               np.zeros((1, 2), dtype=np.int32), np.ones(1, dtype=bool))
    c = topology.Components(records, None, _tables((3, 3)), "faces", "inside", 0.0, 0)
    with pytest.raises(ValueError, match="dropped"):
        c.moments()
