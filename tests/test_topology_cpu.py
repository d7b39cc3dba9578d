"""CPU (no GPU needed): the numpy reference of aegolius_amd.topology (tests/topology_reference.py) proves itself on shapes
whose Betti numbers are known, the 2-D duality holds on random images, the arguments are validated before any device
work, and the header declares the entry points."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import topology_reference as R  # noqa: E402
import topology_shapes as S  # noqa: E402
from aegolius_amd import topology  # noqa: E402

ROOT = os.path.dirname(HERE)


@pytest.mark.parametrize("name", sorted(S.ANALYTIC))
def test_analytic_shapes_have_their_betti_numbers(name):
    field, _, want = S.analytic(name)
    got = R.betti(R.inside(field))
    assert got[:len(want)] == want, (name, got)


def test_a_disc_cut_by_the_border_touches_it():
    x = np.linspace(-1, 1, 65)
    X, Y = np.meshgrid(x, x, indexing="ij")
    c = R.label_field(np.hypot(X - 0.9, Y) - 0.3)
    assert c.count == 1 and c.border.tolist() == [True]
    c = R.label_field(np.hypot(X - 0.2, Y) - 0.3)
    assert c.count == 1 and c.border.tolist() == [False]
    assert c.lower.tolist() == [[29, 23]] and c.upper.tolist() == [[48, 41]] and c.first.tolist() == [29 * 65 + 31]


def test_a_pocket_that_opens_to_the_border_is_no_cavity():
    field, _, want = S.analytic("hollow_sphere")
    assert R.betti(R.inside(field))[:3] == (1, 0, 1)
    x = np.linspace(-1, 1, 33)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    channel = np.maximum(np.hypot(Y, Z) - 0.16, -X)             # a bore along +x from the centre to the grid's face
    assert R.betti(R.inside(np.maximum(field, -channel)))[:3] == (1, 0, 0)


def test_duality_in_2d_on_random_images():
    rng = np.random.default_rng(2024)
    for k in range(200):
        shape = (int(rng.integers(2, 20)), int(rng.integers(2, 20)))
        mask = rng.random(shape) < rng.uniform(0.3, 0.7)
        R.betti(mask)                                          # (asserts holes by labelling == b0 - euler)


def test_checkerboard():
    for shape in ((6, 8), (4, 6, 8), (5, 7)):
        mask = np.indices(shape).sum(axis=0) % 2 == 0
        assert R.label(mask, "faces").count == (mask.size + 1) // 2
        assert R.label(mask, "full").count == 1
        c = R.label(mask, "faces")
        assert np.array_equal(c.first, np.flatnonzero(mask)) and np.all(c.sizes == 1)


def test_canonical_numbering_and_records():
    mask = np.array([[0, 1, 1, 0, 1],
                     [0, 0, 0, 0, 1],
                     [1, 0, 1, 1, 1],
                     [1, 0, 0, 0, 0]], dtype=bool)
    c = R.label(mask, "faces")
    assert c.labels.tolist() == [[-1, 0, 0, -1, 1], [-1, -1, -1, -1, 1], [2, -1, 1, 1, 1], [2, -1, -1, -1, -1]]
    assert c.first.tolist() == [1, 4, 10] and c.sizes.tolist() == [2, 5, 2]
    assert c.lower.tolist() == [[0, 1], [0, 2], [2, 0]] and c.upper.tolist() == [[0, 2], [2, 4], [3, 0]]
    assert c.border.tolist() == [True, True, True]
    assert R.label(mask, "full").count == 3 and R.label(~mask, "faces").count == 1
    assert R.label(np.eye(4, dtype=bool), "full").count == 1 and R.label(~np.eye(4, dtype=bool), "full").count == 1
    assert R.label(np.eye(4, dtype=bool), "faces").count == 4 and R.label(~np.eye(4, dtype=bool), "faces").count == 2
    assert R.cell_counts(mask) == (9, 6, 0, 0)
    assert R.cell_counts(np.ones((2, 3, 4), dtype=bool)) == (24, 46, 29, 6)


def test_argument_validation_needs_no_device():
    ax = np.linspace(-1, 1, 5)
    f = np.ones(125, dtype=np.float32)
    with pytest.raises(ValueError, match="2 or 3 axis tables"):
        topology.label(f, (ax,))
    with pytest.raises(ValueError, match="2 or 3 axis tables"):
        topology.label(f, (ax, ax, ax, ax))
    with pytest.raises(ValueError, match="at least 2"):
        topology.label(f, (ax, ax, ax[:1]))
    with pytest.raises(ValueError, match="strictly increasing"):
        topology.label(f, (ax, ax[::-1], ax))
    with pytest.raises(ValueError, match="NaN"):
        topology.label(f, (ax, ax, ax), level=float("nan"))
    with pytest.raises(ValueError, match="connectivity"):
        topology.label(f, (ax, ax, ax), connectivity="edges")
    with pytest.raises(ValueError, match="region"):
        topology.label(f, (ax, ax, ax), region="border")
    with pytest.raises(ValueError, match="125 values; the axes span 5x5x4 = 100 points"):
        topology.label(f, (ax, ax, ax[:4]))
    with pytest.raises(ValueError, match="125 values"):
        topology.betti(f, (ax, ax))
    with pytest.raises(ValueError, match="125 values"):
        topology.cell_counts(f, (ax, ax[:4]))
    big = np.arange(1291, dtype=np.float32)
    for call in (topology.label, topology.betti, topology.cell_counts):
        with pytest.raises(ValueError, match=r"2\^31 - 1 points"):
            call(f, (big, big, big))
    with pytest.raises(ValueError, match="2 or 3 entries"):
        topology.from_geometry(None, (2,), (9,))
    with pytest.raises(ValueError, match="takes a geometry"):
        topology.from_geometry(f, (2, 2, 2), (5, 5, 5))


def test_header_declares_the_entry_points(built):
    header = open(os.path.join(ROOT, "include", "sdfk.h")).read()
    for name in ("sdfk_label_scratch", "sdfk_field_label", "sdfk_eval_grid_label", "sdfk_label_bits", "sdfk_label_finish",
                 "sdfk_field_cell_counts", "sdfk_eval_grid_cell_counts", "sdfk_label_field"):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in built.SIGNATURES and hasattr(built.lib(), name)
    assert built.lib().sdfk_abi_version() == 1
    # the scratch is sized without a device: at most 1 byte per point and the per-tile and per-axis terms
    n = 257 ** 3
    assert 0.25 * n < built.lib().sdfk_label_scratch(257, 257, 257) <= n + 8 * (n // 8192) + 4 * 3 * 257 + 8192
    assert built.lib().sdfk_label_scratch(130, 130, 1) >= 3 * 256
