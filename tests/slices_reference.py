"""numpy restatement of the definition of aegolius_amd.slices (the test oracle of the plane-stack kernels).

The stack of a field F of shape (L, nu, nv) is mesh_reference.extract(F[l], (U, V), level) per layer, the layers' arrays
one after the other with the vertex ids made global. The section measures follow the module's formulas in float64 from
the float32 vertices, relative to the rectangle's centre, the segments added in their order.
"""
import numpy as np

import mesh_reference


def stack(F, axes, level=0.0):
    """-> (vertices (V, 2) float32, segments (S, 2) int64, vertex offsets (L + 1,), segment offsets (L + 1,))."""
    U, V = (np.asarray(a, dtype=np.float32).ravel() for a in axes)
    F = np.asarray(F, dtype=np.float32).reshape(-1, U.size, V.size)
    verts, segs, voff, soff = [], [], [0], [0]
    for layer in F:
        v, s = mesh_reference.extract(layer, (U, V), level)
        verts.append(v.reshape(-1, 2))
        segs.append(s.reshape(-1, 2) + voff[-1])
        voff.append(voff[-1] + len(v))
        soff.append(soff[-1] + len(s))
    return (np.concatenate(verts).astype(np.float32), np.concatenate(segs).astype(np.int64),
            np.asarray(voff, dtype=np.int64), np.asarray(soff, dtype=np.int64))


def centre(axes):
    U, V = (np.asarray(a, dtype=np.float32).ravel() for a in axes)
    return 0.5 * (float(U[0]) + float(U[-1])), 0.5 * (float(V[0]) + float(V[-1]))


def segment_terms(vertices, segments, axes):
    """Per segment, float64: (t_s, length, (a0 + a1 - 2 ca) t_s / 6, (b0 + b1 - 2 cb) t_s / 6)."""
    ca, cb = centre(axes)
    v = np.asarray(vertices, dtype=np.float32).astype(np.float64)
    s = np.asarray(segments, dtype=np.int64)
    a0, b0, a1, b1 = v[s[:, 0], 0], v[s[:, 0], 1], v[s[:, 1], 0], v[s[:, 1], 1]
    t = (a0 - ca) * (b1 - cb) - (a1 - ca) * (b0 - cb)
    return t, np.hypot(a1 - a0, b1 - b0), (a0 + a1 - 2 * ca) * t / 6.0, (b0 + b1 - 2 * cb) * t / 6.0


def measures(vertices, segments, vertex_offsets, segment_offsets, axes):
    """-> dict of per-layer arrays: area, perimeter, centroid (L, 2), moments (L, 2), segments, border, closed, and
    abs_t (sum of |t_s|, the scale of the rounding error of the area and moment sums). Open layers: NaN area and
    centroid."""
    U, V = (np.asarray(a, dtype=np.float32).ravel() for a in axes)
    ca, cb = centre(axes)
    t, length, ma, mb = segment_terms(vertices, segments, axes)
    v = np.asarray(vertices, dtype=np.float32)
    L = len(vertex_offsets) - 1
    out = {k: np.zeros(L) for k in ("area", "perimeter", "abs_t")}
    out["moments"] = np.zeros((L, 2))
    out["segments"] = np.zeros(L, dtype=np.int64)
    out["border"] = np.zeros(L, dtype=np.int64)
    for l in range(L):
        s = slice(int(segment_offsets[l]), int(segment_offsets[l + 1]))
        mine = v[int(vertex_offsets[l]):int(vertex_offsets[l + 1])]
        out["area"][l] = 0.5 * t[s].sum()
        out["abs_t"][l] = np.abs(t[s]).sum()
        out["perimeter"][l] = length[s].sum()
        out["moments"][l] = (ma[s].sum(), mb[s].sum())
        out["segments"][l] = s.stop - s.start
        out["border"][l] = np.count_nonzero((mine[:, 0] == U[0]) | (mine[:, 0] == U[-1]) | (mine[:, 1] == V[0])
                                            | (mine[:, 1] == V[-1]))
    out["closed"] = out["border"] == 0
    out["area"] = np.where(out["closed"], out["area"], np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["centroid"] = np.asarray((ca, cb)) + out["moments"] / out["area"][:, None]
    return out
