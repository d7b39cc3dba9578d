"""CPU (no GPU needed): the numpy reference of aegolius_amd.layers (tests/layers_reference.py) against answers known by
construction on hand-made stacks; the host half of the module (the candidate reduction, the queries of a LayerGraph) against
the reference; the arguments are refused before anything asks for the GPU; the header declares the entry points."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import aegolius_amd.cores as ns  # noqa: E402
import layers_reference as LR  # noqa: E402
import scenes  # noqa: E402
from aegolius_amd import _engine, layers, slices  # noqa: E402

ROOT = os.path.dirname(HERE)
CONNECTIVITY = ("faces", "full")


def _bridge():
    """Two pillars (layers 0 .. 2) joined by a bridge (layers 3, 4) of 10 columns, 2 over each pillar."""
    m = np.zeros((5, 5, 12), dtype=bool)
    m[:3, 2, 1:3] = True
    m[:3, 2, 9:11] = True
    m[3:, 2, 1:11] = True
    return m


def _floating():
    m = np.zeros((4, 7, 9), dtype=bool)
    m[0] = True
    m[2:, 2:5, 3:6] = True
    return m


def _fork():
    m = np.zeros((4, 5, 11), dtype=bool)
    m[:2, 2, 2:9] = True
    m[2:, 2, 2:4] = True
    m[2:, 2, 7:9] = True
    return m


def _inverted_staircase(L=6, nu=3, nv=10):
    m = np.zeros((L, nu, nv), dtype=bool)
    for l in range(L):
        m[l, :, :2 + l] = True
    return m


def _ids(*arrays):
    return [a.tolist() for a in arrays]


@pytest.mark.parametrize("connectivity", CONNECTIVITY)
def test_two_pillars_and_a_bridge(connectivity):
    g = LR.graph(_bridge(), connectivity)
    assert g.count == 8 and g.layer_offsets.tolist() == [0, 2, 4, 6, 7, 8]
    births, merges, splits, ends = LR.events(g)
    assert _ids(births, merges, splits, ends) == [[], [6], [], []] and LR.islands(g).size == 0
    assert g.child.tolist() == [2, 3, 4, 5, 6, 6, 7] and g.parent.tolist() == [0, 1, 2, 3, 4, 5, 6]
    assert g.overlap.tolist() == [2, 2, 2, 2, 2, 2, 10]
    assert g.overhang[6] == 10 - 4 and g.supported[6] == 4                     # the span between the pillars
    assert g.overhang[7] == 0 and g.overhang[:2].tolist() == [2, 2]             # the base: supported = 0 by definition
    assert not g.border.any() and g.lower[6].tolist() == [3, 2, 1] and g.upper[6].tolist() == [3, 2, 10]
    assert g.first[6] == (3 * 5 + 2) * 12 + 1


@pytest.mark.parametrize("connectivity", CONNECTIVITY)
def test_a_block_floating_above_a_plate(connectivity):
    g = LR.graph(_floating(), connectivity)
    assert g.count == 3 and g.layer_offsets.tolist() == [0, 1, 1, 2, 3]
    assert LR.islands(g).tolist() == [1] and g.layer_of[1] == 2                 # one island, at the block's lowest layer
    assert g.supported.tolist() == [0, 0, 9] and g.overhang.tolist() == [63, 9, 0]
    assert g.border.tolist() == [True, False, False]                          # the plate fills layer 0; the block's top layer is no border
    births, merges, splits, ends = LR.events(g)
    assert _ids(births, merges, splits, ends) == [[1], [], [], [0]]
    assert [a.tolist() for a in LR.per_layer(g)] == [[1, 0, 1, 1], [63, 0, 9, 9], [0, 0, 0, 9], [63, 0, 9, 0], [0, 0, 1, 0]]


@pytest.mark.parametrize("connectivity", CONNECTIVITY)
def test_a_pillar_that_forks(connectivity):
    g = LR.graph(_fork(), connectivity)
    assert g.count == 6
    births, merges, splits, ends = LR.events(g)
    assert _ids(births, merges, splits, ends) == [[], [], [1], []]
    assert g.child.tolist() == [1, 2, 3, 4, 5] and g.parent.tolist() == [0, 1, 1, 2, 3]
    assert g.overhang[1:].tolist() == [0, 0, 0, 0, 0]


def test_an_inverted_staircase_overhangs_by_one_column_per_layer():
    g = LR.graph(_inverted_staircase(), "faces")
    assert g.count == 6 and g.overhang[1:].tolist() == [3] * 5 and g.supported[1:].tolist() == [3 * (2 + l) for l in range(5)]
    assert g.border.all() and LR.islands(g).size == 0


@pytest.mark.parametrize("connectivity", CONNECTIVITY)
def test_all_inside_and_all_outside(connectivity):
    g = LR.graph(np.ones((4, 3, 5), dtype=bool), connectivity)
    assert g.count == 4 and g.layer_offsets.tolist() == [0, 1, 2, 3, 4]
    assert g.overhang.tolist() == [15, 0, 0, 0] and g.overlap.tolist() == [15, 15, 15]
    g = LR.graph(np.zeros((4, 3, 5), dtype=bool), connectivity)
    assert g.count == 0 and g.child.size == 0 and g.layer_offsets.tolist() == [0] * 5
    assert g.first.shape == (0,) and g.lower.shape == (0, 3) and all(a.size == 0 for a in LR.events(g))


def test_diagonal_contacts_join_under_full_only_and_never_across_layers():
    m = np.zeros((3, 4, 4), dtype=bool)
    m[0, 0, 0] = m[0, 1, 1] = True                                             # a diagonal pair in layer 0
    m[1, 1, 2] = True                                                          # diagonal to (0, 1, 1) across layers: no link
    m[2, 1, 2] = True
    faces, full = LR.graph(m, "faces"), LR.graph(m, "full")
    assert (faces.count, full.count) == (4, 3)
    assert full.child.tolist() == [2] and full.parent.tolist() == [1] and LR.islands(full).tolist() == [1]


# ---- the host half of the module against the reference -------------------------------------------------------------------
def _host_graph(mask, connectivity):
    """A LayerGraph from the reference's records and from candidates cut as the kernel cuts them: one per stretch of a
    row, here split further and shuffled — combine() must not depend on either."""
    want = LR.graph(mask, connectivity)
    L, nu, nv = mask.shape
    above, below = want.labels[1:].reshape(-1), want.labels[:-1].reshape(-1)
    both = np.flatnonzero((above >= 0) & (below >= 0))
    order = np.random.default_rng(7).permutation(both.size)
    child, parent = above[both][order].astype(np.int64), below[both][order].astype(np.int64)
    links = layers.combine(child, parent, np.ones(child.size, dtype=np.int32))
    tables = [np.arange(s, dtype=np.float32) for s in mask.shape]
    records = (want.first, want.sizes, want.lower, want.upper, want.border)
    supported = np.bincount(child, minlength=want.count)
    return layers.LayerGraph(records, None, tables, connectivity, 0.0, 0, links, supported), want


@pytest.mark.parametrize("connectivity", CONNECTIVITY)
def test_the_queries_of_a_graph_equal_the_reference(connectivity):
    rng = np.random.default_rng(11)
    for mask in (_bridge(), _floating(), _fork(), _inverted_staircase(), rng.random((6, 9, 11)) < 0.45, np.zeros((3, 2, 2), dtype=bool)):
        got, want = _host_graph(mask, connectivity)
        for name in ("layer_offsets", "layer_of", "child", "parent", "overlap", "supported", "overhang"):
            a, b = getattr(got, name), getattr(want, name)
            assert a.dtype == np.int64 and a.shape == b.shape, name
            np.testing.assert_array_equal(a, b, err_msg=name)
        np.testing.assert_array_equal(got.islands(), LR.islands(want))
        for a, b in zip(got.events(), LR.events(want)):
            np.testing.assert_array_equal(a, b)
        for a, b in zip(got.per_layer(), LR.per_layer(want)):
            assert a.dtype == np.int64
            np.testing.assert_array_equal(a, b)
        for c in range(want.count):
            np.testing.assert_array_equal(got.parents(c), want.parent[want.child == c])
            np.testing.assert_array_equal(got.children(c), want.child[want.parent == c])
        np.testing.assert_array_equal(got.overhang_area(), got.per_layer().overhang.astype(np.float64))   # (du = dv = 1)
        with pytest.raises(ValueError, match="dropped"):
            got.labels_host()


def test_overhang_area_needs_uniform_in_plane_tables():
    got, _ = _host_graph(_bridge(), "faces")
    bent = [np.arange(5.0), np.array([0, 1, 2, 3, 5.0]), np.arange(12.0) * 0.5]
    uneven = layers.LayerGraph((got.first, got.sizes, got.lower, got.upper, got.border), None, got.axes, "faces", 0.0, 0,
                               (got.child, got.parent, got.overlap), got.supported, given=bent)
    with pytest.raises(ValueError, match="not uniform"):
        uneven.overhang_area()
    heights_bent = [np.array([0, 1, 2, 3, 5.0]), np.arange(5.0) * 0.25, np.arange(12.0) * 0.5]      # (heights may be anything)
    ok = layers.LayerGraph((got.first, got.sizes, got.lower, got.upper, got.border), None, got.axes, "faces", 0.0, 0,
                           (got.child, got.parent, got.overlap), got.supported, given=heights_bent)
    np.testing.assert_array_equal(ok.overhang_area(), got.per_layer().overhang * 0.125)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_arguments_are_refused_before_the_gpu_is_asked_for(monkeypatch):
    def asked():
        raise AssertionError("the GPU was asked for")
    monkeypatch.setattr(_engine, "require_gpu", asked)
    ax = np.linspace(-1, 1, 5)
    f = np.ones(125, dtype=np.float32)
    sphere = ns.Sphere(0.5)
    with pytest.raises(ValueError, match="heights has 1 point"):
        layers.graph(f[:25], (ax, ax), ax[:1])
    with pytest.raises(ValueError, match="heights has 1 point"):
        layers.graph(sphere, (ax, ax), ax[:1])
    with pytest.raises(ValueError, match="axis V is not strictly increasing"):
        layers.graph(f, (ax, ax[::-1]), ax)
    with pytest.raises(ValueError, match="heights is not strictly increasing"):
        layers.graph(sphere, (ax, ax), [0.0, 0.5, 0.5])
    with pytest.raises(ValueError, match="connectivity"):
        layers.graph(f, (ax, ax), ax, connectivity="edges")
    with pytest.raises(ValueError, match="a Frame goes with a geometry"):
        layers.graph(f, (ax, ax), ax, normal=slices.Frame())
    with pytest.raises(ValueError, match="normal: 0, 1, 2 or a Frame"):
        layers.graph(f, (ax, ax), ax, normal=3)
    with pytest.raises(ValueError, match="NaN"):
        layers.graph(f, (ax, ax), ax, level=float("nan"))
    build, key = scenes.GRID_SCENES["grid_conv_sphere_3x3x3"]
    with pytest.raises(ValueError, match="conv_averaging.*staged tree"):
        layers.graph(build(ns, scenes.GRIDS[key][1]), (ax, ax), ax)
    big = np.arange(1291, dtype=np.float32)
    for source in (f, sphere):
        with pytest.raises(ValueError, match=r"2\^31 - 1 points"):
            layers.graph(source, (big, big), big)
    with pytest.raises(ValueError, match="125 values; the stack spans 4x5x5 = 100 points"):
        layers.graph(f, (ax, ax), ax[:4])
    with pytest.raises(ValueError, match="two in-plane tables"):
        layers.graph(f, (ax, ax, ax), ax)
    with pytest.raises(ValueError, match="3 entries"):
        layers.from_geometry(sphere, (2, 2), (9, 9))
    with pytest.raises(ValueError, match="takes a geometry"):
        layers.from_geometry(f, (2, 2, 2), (5, 5, 5))


def test_header_declares_the_entry_points(built):
    header = open(os.path.join(ROOT, "include", "sdfk.h")).read()
    for name in ("sdfk_field_layer_label", "sdfk_eval_grid_layer_label", "sdfk_layer_label_bits", "sdfk_layer_label_finish",
                 "sdfk_layer_links", "sdfk_layer_links_finish"):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in built.SIGNATURES and hasattr(built.lib(), name)
