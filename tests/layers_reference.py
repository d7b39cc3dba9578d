"""numpy reference of aegolius_amd.layers (its module text states the definitions): every layer of a boolean (L, nu, nv)
array labelled on its own by topology_reference.label, the ids offset layer by layer, the in-plane border of the 2-D
labelling; the links by np.unique over the stacked label pairs of consecutive layers; supported, overhang, islands,
events and layer totals derived from those. No GPU."""
import numpy as np

import topology_reference as R


class Graph:
    pass


def graph(mask, connectivity="faces"):
    """-> Graph with labels (int32, the mask's shape, -1 off the mask), count, first, sizes, lower, upper, border,
    layer_offsets, layer_of, child, parent, overlap, supported, overhang (the module text of aegolius_amd.layers)."""
    mask = np.asarray(mask, dtype=bool)
    L, nu, nv = mask.shape
    g = Graph()
    g.labels = np.full(mask.shape, -1, dtype=np.int32)
    offsets, parts = [0], []
    for l in range(L):
        c = R.label(mask[l], connectivity)
        g.labels[l] = np.where(c.labels >= 0, c.labels + offsets[-1], -1)
        layer = np.full((c.count, 1), l, dtype=np.int32)
        parts.append((c.first + l * nu * nv, c.sizes, np.hstack([layer, c.lower]), np.hstack([layer, c.upper]), c.border))
        offsets.append(offsets[-1] + c.count)
    g.count = offsets[-1]
    g.layer_offsets = np.asarray(offsets, dtype=np.int64)
    g.first = np.concatenate([p[0] for p in parts]).astype(np.int64)
    g.sizes = np.concatenate([p[1] for p in parts]).astype(np.int64)
    g.lower = np.concatenate([p[2] for p in parts]).astype(np.int32).reshape(-1, 3)
    g.upper = np.concatenate([p[3] for p in parts]).astype(np.int32).reshape(-1, 3)
    g.border = np.concatenate([p[4] for p in parts]).astype(bool)
    g.layer_of = np.repeat(np.arange(L, dtype=np.int64), np.diff(g.layer_offsets))
    above, below = g.labels[1:].ravel().astype(np.int64), g.labels[:-1].ravel().astype(np.int64)
    both = (above >= 0) & (below >= 0)
    pairs, counts = np.unique(np.stack([above[both], below[both]], axis=1), axis=0, return_counts=True)
    g.child, g.parent = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
    g.overlap = counts.astype(np.int64)
    g.supported = np.zeros(g.count, dtype=np.int64)
    np.add.at(g.supported, g.child, g.overlap)
    g.overhang = g.sizes - g.supported
    return g


def islands(g):
    return np.flatnonzero((g.supported == 0) & (g.layer_of >= 1)).astype(np.int64)


def events(g):
    """-> (births, merges, splits, ends), ascending ids."""
    L = len(g.layer_offsets) - 1
    parents = np.bincount(g.child, minlength=g.count)
    children = np.bincount(g.parent, minlength=g.count)
    return (np.flatnonzero((parents == 0) & (g.layer_of >= 1)), np.flatnonzero(parents >= 2), np.flatnonzero(children >= 2),
            np.flatnonzero((children == 0) & (g.layer_of < L - 1)))


def per_layer(g):
    """-> (components, inside, supported, overhang, islands), (L,) int64 each."""
    L = len(g.layer_offsets) - 1
    def total(values):
        return np.array([values[g.layer_offsets[l]:g.layer_offsets[l + 1]].sum() for l in range(L)], dtype=np.int64)
    alone = np.zeros(g.count, dtype=np.int64)
    alone[islands(g)] = 1
    return np.diff(g.layer_offsets), total(g.sizes), total(g.supported), total(g.overhang), total(alone)
