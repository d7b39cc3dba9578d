"""float64 restatement of the projection kernel (csrc/sdfk_project.inc) on the CPU oracle.

The same iteration, the same statuses in the same order, the same stall threshold; the field is the oracle's (float64),
its gradient the oracle's central difference at h = 1e-6, and q is rounded to float32 after every step, as the kernel
holds it. `smooth` marks the points whose every iterate passed the kink filter of tests/test_gpu_autodiff.py: the
differences at h and h / 8 agree to 1e-7 — where they do not, the iterate sits on a crease and the analytic gradient of
the kernel may legitimately be the other side's.
"""
import numpy as np

from aegolius_amd import workloads
from oracle import sdf_oracle

CONVERGED, MAXITER, STALLED, NONFINITE = 0, 1, 2, 3
GMIN2 = float(np.float32(1e-24))
H = 1e-6
SCENES = ("cfg2", "cfg5", "cfg3", "cfg4")
CAP = 0.01                   # share of the points that may end not CONVERGED (the reference's worst share: 0.42 %, cfg 4)


def scene(ns, name):
    """-> (geometry, box sizes) of a BASELINE config."""
    geo, size, _desc = workloads.build(name, ns)
    return geo, tuple(float(s) for s in size)


def scene_points(size, n=4096, seed=5):
    """n uniform points in the box of `size` (2 or 3 entries, centred; z = 0 for 2 entries), as float32 values."""
    rng = np.random.default_rng(seed)
    p = np.zeros((3, n))
    for a, s in enumerate(size):
        p[a] = rng.uniform(-s / 2, s / 2, n)
    return p.astype(np.float32)


def gradient(geo, q, h=H):
    """Central difference of the oracle at q (3, n) float64 -> (3, n)."""
    g = np.zeros_like(q)
    for a in range(3):
        d = np.zeros((3, 1))
        d[a] = h
        g[a] = (sdf_oracle.evaluate(geo, q + d) - sdf_oracle.evaluate(geo, q - d)) / (2 * h)
    return g


def project(geo, p, level=0.0, tol=1e-5, max_iter=32, relax=1.0, kink_filter=False):
    """-> dict(points (3, n) float32, values, gradients, start (float64), iterations, status (uint8), smooth (bool))."""
    level, tol, relax = float(np.float32(level)), float(np.float32(tol)), float(np.float32(relax))
    q = np.array(p, dtype=np.float32).astype(np.float64)
    n = q.shape[1]
    status = np.full(n, -1, dtype=np.int64)
    it = np.zeros(n, dtype=np.int64)
    f = np.zeros(n)
    g = np.zeros((3, n))
    start = np.zeros(n)
    smooth = np.ones(n, dtype=bool)
    for trip in range(max_iter + 1):
        act = np.flatnonzero(status < 0)
        if act.size == 0:
            break
        qa = q[:, act]
        with np.errstate(all="ignore"):
            fa = sdf_oracle.evaluate(geo, qa)
            ga = gradient(geo, qa)
            f[act], g[:, act] = fa, ga
            if trip == 0:
                start[:] = f
            r = fa - level
            g2 = (ga[0] * ga[0] + ga[1] * ga[1]) + ga[2] * ga[2]
            st = np.full(act.size, -1, dtype=np.int64)
            st[~(np.abs(r) <= np.finfo(np.float32).max)] = NONFINITE
            st[(st < 0) & (np.abs(r) <= tol)] = CONVERGED
            if trip == max_iter:
                st[st < 0] = MAXITER
            st[(st < 0) & ~(g2 >= GMIN2)] = STALLED
            go = st < 0
            if kink_filter and go.any():
                g8 = gradient(geo, qa[:, go], H / 8)
                ok = np.all(np.abs(ga[:, go] - g8) <= 1e-7 * np.maximum(1.0, np.abs(ga[:, go])), axis=0)
                smooth[act[go]] &= ok
            s = relax * (r[go] / g2[go])
            q[:, act[go]] = (qa[:, go] - s * ga[:, go]).astype(np.float32).astype(np.float64)
            it[act[go]] += 1
            status[act] = st
    return dict(points=q.astype(np.float32), values=f, gradients=g, start=start, iterations=it.astype(np.uint8),
                status=status.astype(np.uint8), smooth=smooth)


def step_f32(p, f, g, level, tol, relax=1.0):
    """ONE trip of the kernel in numpy float32, operation for operation, from the kernel's own f (n,) and g (3, n) at p
    (3, n): -> (q, status or -1 where the point stepped). The kernel's float expressions, in its order."""
    p, f, g = np.asarray(p, np.float32), np.asarray(f, np.float32), np.asarray(g, np.float32)
    level, tol, relax = np.float32(level), np.float32(tol), np.float32(relax)
    with np.errstate(all="ignore"):
        r = f - level
        g2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
        st = np.full(f.shape, -1, dtype=np.int64)
        st[~(np.abs(r) <= np.finfo(np.float32).max)] = NONFINITE
        st[(st < 0) & (np.abs(r) <= tol)] = CONVERGED
        st[(st < 0) & ~(g2 >= np.float32(1e-24))] = STALLED
        s = relax * (r / g2)
        q = np.stack([p[0] - s * g[0], p[1] - s * g[1], p[2] - s * g[2]]).astype(np.float32)
    q[:, st >= 0] = p[:, st >= 0]
    return q, st
