"""numpy reference of aegolius_amd.topology (its module text states the definitions): labelling of a boolean array by
repeated min-propagation over the neighbour pairs, canonical numbering by the smallest linear index, the records, the cell
counts by sliced ANDs and the Betti numbers. No GPU, no scipy."""
import itertools

import numpy as np


def inside(field, level=0.0):
    """The mesh's rule: f <= level as float32, NaN outside."""
    with np.errstate(invalid="ignore"):
        return np.asarray(field, dtype=np.float32) <= np.float32(level)


def offsets(dims, connectivity):
    """The backward half of the neighbourhood: index offsets lexicographically below zero."""
    out = []
    for d in itertools.product((-1, 0, 1), repeat=dims):
        if d >= (0,) * dims:
            continue
        if connectivity == "faces" and sum(abs(x) for x in d) != 1:
            continue
        out.append(d)
    if connectivity not in ("faces", "full"):
        raise ValueError(connectivity)
    return out


def _pairs(mask, d):
    """Linear indices (p, q) of the points p and q = p + d that are both set."""
    idx = np.arange(mask.size, dtype=np.int64).reshape(mask.shape)
    a = tuple(slice(max(0, -x), mask.shape[k] - max(0, x)) for k, x in enumerate(d))
    b = tuple(slice(max(0, x), mask.shape[k] - max(0, -x)) for k, x in enumerate(d))
    both = mask[a] & mask[b]
    return idx[a][both], idx[b][both]


def roots(mask, connectivity):
    """Per point the smallest linear index of its component (-1 off the mask): every pair of neighbours hooks the larger
    of its two roots under the smaller, pointers are jumped until they are roots, until nothing changes."""
    mask = np.asarray(mask, dtype=bool)
    parent = np.arange(mask.size, dtype=np.int64)
    pairs = [_pairs(mask, d) for d in offsets(mask.ndim, connectivity)]
    pairs = [(p, q) for p, q in pairs if p.size]
    while True:
        changed = False
        for p, q in pairs:
            rp, rq = parent[p], parent[q]
            lo, hi = np.minimum(rp, rq), np.maximum(rp, rq)
            differ = lo != hi
            if differ.any():
                np.minimum.at(parent, hi[differ], lo[differ])
                changed = True
            while True:
                nxt = parent[parent]
                if np.array_equal(nxt, parent):
                    break
                parent = nxt
        if not changed:
            break
    out = parent.reshape(mask.shape)
    return np.where(mask, out, -1)


class Components:
    pass


def label(mask, connectivity="faces"):
    """-> Components with labels (int32, the mask's shape, -1 off the mask), count, first, sizes, lower, upper, border."""
    mask = np.asarray(mask, dtype=bool)
    root = roots(mask, connectivity)
    first = np.unique(root[mask])                              # ascending: the canonical numbering
    labels = np.full(mask.shape, -1, dtype=np.int32)
    labels[mask] = np.searchsorted(first, root[mask]).astype(np.int32)
    c = Components()
    c.labels, c.count, c.first = labels, int(first.size), first.astype(np.int64)
    K, D = c.count, mask.ndim
    c.sizes = np.bincount(labels[mask], minlength=K).astype(np.int64)
    c.lower = np.zeros((K, D), dtype=np.int32)
    c.upper = np.zeros((K, D), dtype=np.int32)
    c.border = np.zeros(K, dtype=bool)
    coords = np.nonzero(mask)
    ids = labels[mask]
    for a in range(D):
        lo = np.full(K, np.iinfo(np.int32).max, dtype=np.int64)
        hi = np.full(K, -1, dtype=np.int64)
        np.minimum.at(lo, ids, coords[a])
        np.maximum.at(hi, ids, coords[a])
        c.lower[:, a], c.upper[:, a] = lo, hi
        c.border |= (lo == 0) | (hi == mask.shape[a] - 1)
    return c


def label_field(field, level=0.0, connectivity="faces", region="inside"):
    m = inside(field, level)
    if region not in ("inside", "outside"):
        raise ValueError(region)
    return label(m if region == "inside" else ~m, connectivity)


def cell_counts(mask):
    """(V, E, F, C): points, edges, squares and cubes of the grid whose corners are all set (C = 0 in 2-D)."""
    mask = np.asarray(mask, dtype=bool)
    D = mask.ndim
    counts = [0, 0, 0, 0]
    for axes in itertools.chain.from_iterable(itertools.combinations(range(D), k) for k in range(D + 1)):
        cell = np.ones([s - (1 if a in axes else 0) for a, s in enumerate(mask.shape)], dtype=bool)
        for corner in itertools.product((0, 1), repeat=len(axes)):
            sl = [slice(None)] * D
            for a in range(D):
                if a in axes:
                    o = corner[axes.index(a)]
                    sl[a] = slice(o, mask.shape[a] - 1 + o)
            cell &= mask[tuple(sl)]
        counts[len(axes)] += int(np.count_nonzero(cell))
    return tuple(counts)


def betti(mask):
    """(b0, b1, b2, euler) of the cubical complex the set points span; 2-D: b2 = 0 and b1 is checked against the holes."""
    mask = np.asarray(mask, dtype=bool)
    V, E, F, C = cell_counts(mask)
    euler = V - E + F - C
    b0 = label(mask, "faces").count
    enclosed = int(np.count_nonzero(~label(~mask, "full").border))
    if mask.ndim == 3:
        return b0, b0 + enclosed - euler, enclosed, euler
    assert b0 - euler == enclosed, (b0, euler, enclosed)
    return b0, enclosed, 0, euler
