"""numpy reference of the component moments of aegolius_amd.topology (its module text states the sums): from a label
array, per id the sums of 1, i_a and i_a i_b over its points, added in uint64 with np.add.at — integers all the way
(np.bincount(weights=...) would add in float64, which is inexact above 2^53). No GPU."""
import numpy as np

PAIRS = {2: ((0, 0), (0, 1), (1, 1)), 3: ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))}


def sums(labels, count):
    """labels: an integer array of the grid's shape (2-D or 3-D), -1 off the components, ids 0 .. count - 1 ->
    (count, 10) uint64 (N, I0, I1, I2, I00, I01, I02, I11, I12, I22), 2-D: (count, 6) (N, I0, I1, I00, I01, I11)."""
    labels = np.asarray(labels)
    d = labels.ndim
    out = np.zeros((int(count), 1 + d + len(PAIRS[d])), dtype=np.uint64)
    on = labels >= 0
    ids = labels[on].astype(np.int64)
    idx = [i.astype(np.uint64) for i in np.nonzero(on)]
    np.add.at(out[:, 0], ids, np.uint64(1))
    for a in range(d):
        np.add.at(out[:, 1 + a], ids, idx[a])
    for t, (a, b) in enumerate(PAIRS[d]):                       # (one product at a time: a 513^3 grid has 1e8 points)
        np.add.at(out[:, 1 + d + t], ids, idx[a] * idx[b])
    return out
