"""numpy implementation of the isosurface / contour definition of aegolius_amd.mesh (the test oracle of the GPU kernels).

Vectorised, but it follows the definition step by step: inside bits, crossing edges in (point, axis) order, float32
positions in the definition's operation order, cases from the generated table, triangles in (cell, table) order.
Also: manifold and orientation checks on the result.
"""
import numpy as np

from aegolius_amd import _mctable


def _inside(f, level):
    f = np.asarray(f, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (f <= np.float32(level)) & ~np.isnan(f)


def _vertices(f, ins, tables, level, strides, shape):
    """Crossing-edge keys (point * D + axis, ascending) and their float32 positions."""
    D = len(shape)
    n = ins.size
    flat = ins.ravel()
    keys = []
    for a in range(D):
        sl_lo = [slice(None)] * D
        sl_lo[a] = slice(0, shape[a] - 1)
        sl_hi = [slice(None)] * D
        sl_hi[a] = slice(1, None)
        cross = np.zeros(shape, dtype=bool)
        cross[tuple(sl_lo)] = ins[tuple(sl_lo)] != ins[tuple(sl_hi)]
        keys.append(np.flatnonzero(cross.ravel()) * D + a)
    key = np.sort(np.concatenate(keys)) if keys else np.zeros(0, np.int64)
    p, a = key // D, key % D
    ff = np.asarray(f, dtype=np.float32).ravel()
    idx = np.stack(np.unravel_index(p, shape)) if len(p) else np.zeros((D, 0), np.int64)
    pos = np.empty((len(p), D), dtype=np.float32)
    for o in range(D):
        pos[:, o] = tables[o][idx[o]]
    lv = np.float32(level)
    svec = np.asarray(strides, dtype=np.int64)
    fa = ff[p]
    fb = ff[p + svec[a]]
    for o in range(D):
        m = a == o
        if not m.any():
            continue
        xa = tables[o][idx[o][m]]
        xb = tables[o][idx[o][m] + 1]
        fa_, fb_ = fa[m], fb[m]
        with np.errstate(all="ignore"):
            t = (lv - fa_) / (fb_ - fa_)
            x = xa + t * (xb - xa)
        x = np.where(np.isnan(fa_), xb, np.where(np.isnan(fb_), xa, x)).astype(np.float32)
        pos[m, o] = x
    assert n == ff.size
    return key, pos


def extract(f, axes, level=0.0):
    """-> (vertices (V, D) float32, faces (F, D) int64) for D = len(axes) = 3 (triangles) or 2 (segments)."""
    tables = [np.asarray(a, dtype=np.float32).ravel() for a in axes]
    D = len(tables)
    shape = tuple(t.size for t in tables)
    f = np.asarray(f, dtype=np.float32).reshape(shape)
    ins = _inside(f, level)
    strides = [int(np.prod(shape[a + 1:])) for a in range(D)]
    key, pos = _vertices(f, ins, tables, level, strides, shape)
    # cell cases
    case = np.zeros(tuple(s - 1 for s in shape), dtype=np.int32)
    for c in range(1 << D):
        off = [(c >> (D - 1 - a)) & 1 for a in range(D)]
        sl = tuple(slice(o, o + s - 1) for o, s in zip(off, shape))
        case |= ins[sl].astype(np.int32) << c
    t = _mctable.tables()
    if D == 3:
        ntab = np.array([len(x) for x in t["tri"]], dtype=np.int64)
        tab = np.zeros((256, t["tmax"], 3), dtype=np.int64)
        for c, x in enumerate(t["tri"]):
            if x:
                tab[c, :len(x)] = x
    else:
        ntab = np.array([len(x) for x in t["seg"]], dtype=np.int64)
        tab = np.zeros((16, t["smax"], 2), dtype=np.int64)
        for c, x in enumerate(t["seg"]):
            if x:
                tab[c, :len(x)] = x
    cflat = case.ravel()
    cells = np.flatnonzero(ntab[cflat] > 0)
    cc = cflat[cells]
    cnt = ntab[cc]
    rep = np.repeat(np.arange(len(cells)), cnt)
    within = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    edges = tab[cc[rep], within]                         # (F, D) edge ids
    cidx = np.stack(np.unravel_index(cells[rep], case.shape)) if len(rep) else np.zeros((D, 0), np.int64)
    p = np.zeros(len(rep), dtype=np.int64)
    for a in range(D):
        p += cidx[a] * strides[a]
    faces = np.empty((len(rep), D), dtype=np.int64)
    for col in range(D):
        e = edges[:, col]
        q = p.copy()
        if D == 3:
            a = e >> 2
            o1 = np.where(a == 0, 1, 0)
            o2 = np.where(a == 2, 1, 2)
            sv = np.asarray(strides)
            q += np.where(e & 2, sv[o1], 0) + np.where(e & 1, sv[o2], 0)
        else:
            a = e >> 1
            q += np.where(e & 1, np.asarray(strides)[1 - a], 0)
        k = q * D + a
        vid = np.searchsorted(key, k)
        assert np.all(key[np.minimum(vid, len(key) - 1)] == k), "a face uses an edge without a vertex"
        faces[:, col] = vid
    return pos, faces


# ---- checks ---------------------------------------------------------------------------------------------------------------
def directed_edges(faces):
    f = np.asarray(faces, dtype=np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def is_closed_oriented_manifold(faces):
    """Every directed edge once, and its reverse once: closed, consistently oriented. (Vertex links are not checked.)"""
    d = directed_edges(faces)
    if len(d) == 0:
        return True
    code = d[:, 0] * (d.max() + 1) + d[:, 1]
    rev = d[:, 1] * (d.max() + 1) + d[:, 0]
    if np.unique(code).size != code.size:
        return False
    return bool(np.all(np.isin(rev, code)))


def euler_characteristic(vertices, faces):
    d = directed_edges(faces)
    und = np.unique(np.sort(d, axis=1), axis=0)
    return len(vertices) - len(und) + len(faces)


def signed_volume(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    t = v[np.asarray(faces)]
    return float(np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6.0)
