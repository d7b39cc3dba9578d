"""Projection of points onto a level set of a geometry, on the GPU (kernel: csrc/sdfk_project.inc).

    from aegolius_amd import surface
    sp = surface.project(geometry, co)              # co: (3, N) host array, generate_grid output or a DeviceVectorField
    sp.points, sp.normals(), sp.distance(), sp.converged

Every point runs Newton's iteration on f - level with the exact gradient of the dual kernel (autodiff's point mode),

    q <- q - relax (f(q) - level) ∇f(q) / |∇f(q)|²,

all iterations in ONE launch: 12 B per point in, at most 36 B out, whatever the iteration count. The program is create()'s
own (the default lowering), so `values` are what create() returns at `points`, bit for bit.

What it promises: a point with status CONVERGED has |f - level| <= tol. What it does not: that point is the NEAREST point
of the level set only where f is an exact distance field (there one step suffices); across a concave crease the iteration
can alternate between the two sides, which is reported as MAXITER, never hidden; where the gradient vanishes (a centre,
an axis, a flat map) the point is STALLED and stays where it was.
"""
import ctypes

import numpy as np

from . import _engine
from ._eval import config, device_coords
from .autodiff import _host, _lower, _program

CONVERGED, MAXITER, STALLED, NONFINITE = 0, 1, 2, 3
STATUS_NAMES = ("CONVERGED", "MAXITER", "STALLED", "NONFINITE")
MAX_ITER_LIMIT = 255


class SurfacePoints:
    """What project() returns. `points` (3, N), `values` (N,) the field at them, `gradients` (3, N) its gradient at
    them, `start` (N,) the field at the input points: float32 host arrays, or with resident=True a DeviceVectorField /
    DeviceField each (numpy() downloads one). `iterations`, `status` (N,) uint8 and `origin` (3, N) float32 — the input
    points, None for resident input — are host arrays."""

    def __init__(self, points, values, gradients, start, iterations, status, origin=None, level=0.0, tol=0.0):
        self.points, self.values, self.gradients, self.start = points, values, gradients, start
        self.iterations, self.status, self.origin = iterations, status, origin
        self.level, self.tol = float(level), float(tol)

    def __repr__(self):
        counts = np.bincount(np.asarray(self.status, dtype=np.int64), minlength=4)
        return "SurfacePoints(%d points: %s)" % (len(self.status), ", ".join(
            "%d %s" % (c, n.lower()) for c, n in zip(counts, STATUS_NAMES) if c))

    @property
    def converged(self):
        return np.asarray(self.status) == CONVERGED

    @staticmethod
    def _array(x):
        return x.numpy() if isinstance(x, _engine.DeviceBuffer) else np.asarray(x)

    def normals(self):
        """Unit gradients (N, 3) float32, zero where |g| = 0 (the host arithmetic of Mesh.compute_normals)."""
        g = np.asarray(self._array(self.gradients), dtype=np.float64).reshape(3, -1).T
        norm = np.linalg.norm(g, axis=1, keepdims=True)
        return np.ascontiguousarray(np.divide(g, norm, out=np.zeros_like(g), where=norm > 0), dtype=np.float32)

    def distance(self, origin=None):
        """|q - p| per point, float64 on the host. `origin`: the input points, needed only when they were resident."""
        p = self.origin if origin is None else origin
        if p is None:
            raise ValueError("distance: the input points were resident; pass them as `origin`")
        p = np.asarray(self._array(p), dtype=np.float64).reshape(3, -1)
        q = np.asarray(self._array(self.points), dtype=np.float64).reshape(3, -1)
        if p.shape != q.shape:
            raise ValueError("distance: %d input points, %d projected points" % (p.shape[1], q.shape[1]))
        return np.sqrt(np.sum((q - p) ** 2, axis=0))

    def free(self):
        """Release the device rows of a resident result."""
        for x in (self.points, self.values, self.gradients, self.start):
            if isinstance(x, _engine.DeviceBuffer):
                x.free()


def _arguments(level, tol, max_iter, relax):
    with np.errstate(over="ignore"):                            # (a level beyond float32 becomes inf and is refused below)
        level, tol, relax = float(np.float32(level)), float(np.float32(tol)), float(np.float32(relax))
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)):
        raise TypeError("project: max_iter is an integer; got %r" % (max_iter,))
    if not 0 <= max_iter <= MAX_ITER_LIMIT:
        raise ValueError("project: max_iter must be in 0 .. %d; got %d" % (MAX_ITER_LIMIT, max_iter))
    if not np.isfinite(level):
        raise ValueError("project: the level must be finite; got %r" % (level,))
    if not tol >= 0.0:
        raise ValueError("project: tol must be >= 0; got %r" % (tol,))
    if not (np.isfinite(relax) and 0.0 < relax <= 1.0):
        raise ValueError("project: relax must be in (0, 1]; got %r" % (relax,))
    return level, tol, int(max_iter), relax


def project(geometry, co, level=0.0, tol=1e-5, max_iter=32, relax=1.0, resident=False):
    """Move every point of `co` onto {f = level} of `geometry` by Newton's iteration -> SurfacePoints.

    `co`: what autodiff.value_and_grad_points accepts. `tol`: a point is CONVERGED when |f - level| <= tol (float32).
    `max_iter` (0 .. 255): steps a point may take; one that has not converged by then is MAXITER. `relax` in (0, 1]
    scales every step. resident=True leaves the float rows on the device. Raises autodiff.UnsupportedOpError for trees
    without a dual rule or that need a staged evaluation."""
    level, tol, max_iter, relax = _arguments(level, tol, max_iter, relax)
    low, origin = _lower(geometry, shortcuts=True)
    prog = _program(low, origin)
    _engine.require_gpu()
    L = _engine.lib()
    vp = _engine._vp
    _engine.check(L.sdfk_set_device(config.device), "sdfk_set_device")
    made = []
    try:
        with device_coords(co, "project") as coords:
            n = coords.n
            points = _engine.DeviceVectorField(n, config.device)
            made.append(points)
            grads = _engine.DeviceVectorField(n, config.device)
            made.append(grads)
            values = _engine.DeviceField(n, config.device)
            made.append(values)
            start = _engine.DeviceField(n, config.device)
            made.append(start)
            info = np.empty(n, dtype=np.int32)
            with _engine.DeviceBuffer(4 * n, what="project status") as d_info:
                _engine.check(L.sdfk_project_points_device(prog.handle, vp(coords.ptr), n, coords.stride, level, tol,
                                                           max_iter, relax, points.at(), points.stride, values.at(),
                                                           grads.at(), grads.stride, start.at(), d_info.at(), None),
                              "sdfk_project_points_device")
                _engine.check(L.sdfk_sync(None), "sdfk_sync")
                d_info.download(info)
        origin_pts = None if isinstance(co, _engine.DeviceVectorField) else _engine.host_coords(co, np.float32)
        status = (info & 255).astype(np.uint8)
        iterations = ((info >> 8) & 255).astype(np.uint8)
        if not resident:
            host = [points.numpy(), values.numpy(), grads.numpy(), start.numpy()]
            for x in made:
                x.free()
            points, values, grads, start = host
        return SurfacePoints(points, values, grads, start, iterations, status, origin_pts, level, tol)
    except BaseException:
        for x in made:
            x.free()
        raise


def _project_vertices(vertices, geometry, level, kw, dims):
    """The in-place part of Mesh.project / Contour.project -> (SurfacePoints, moved vertices (V, dims), normals (V, 3))."""
    if kw.get("resident"):
        raise ValueError("project: a mesh's vertices live on the host; resident=True is not accepted")
    v = np.asarray(vertices, dtype=np.float32)
    co = np.zeros((3, len(v)), dtype=np.float32)
    co[:dims] = v.T[:dims]
    sp = project(geometry, co, level=level, **kw)
    ok = sp.converged
    moved = np.array(v, dtype=np.float32)
    moved[ok] = sp.points.T[ok][:, :dims]
    return sp, moved, sp.normals()
