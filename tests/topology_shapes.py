"""Shapes whose Betti numbers are known, for the topology tests: each as a numpy field on its grid (the CPU tests) and as
a geometry of the package (the GPU tests). Every feature — wall, tube, hole, gap — is at least 3 grid spacings thick, so
that the cubical complex of the inside points has the topology of the solid."""
import numpy as np


def _grid(size, resolution):
    axes = [np.linspace(-s / 2, s / 2, r) for s, r in zip(size, resolution)]
    return np.meshgrid(*axes, indexing="ij")


def _torus(X, Y, Z, R, r):
    return np.hypot(np.hypot(X, Y) - R, Z) - r


def _sphere(X, Y, Z):
    return np.sqrt(X * X + Y * Y + Z * Z) - 0.6


def _two_spheres(X, Y, Z):
    return np.minimum(np.sqrt((X - 0.5) ** 2 + Y * Y + Z * Z), np.sqrt((X + 0.5) ** 2 + Y * Y + Z * Z)) - 0.3


def _linked_tori(X, Y, Z):
    # one ring in the xy plane around (-0.25, 0, 0), one in the xz plane around (0.25, 0, 0): each passes through the other
    return np.minimum(_torus(X + 0.25, Y, Z, 0.45, 0.1), _torus(X - 0.25, Z, Y, 0.45, 0.1))


def _hollow_sphere(X, Y, Z):
    return np.abs(np.sqrt(X * X + Y * Y + Z * Z) - 0.55) - 0.15


def _annulus(X, Y):
    return np.abs(np.hypot(X, Y) - 0.5) - 0.15


def _geo_sphere(ns):
    return ns.Sphere(0.6)


def _geo_two_spheres(ns):
    a, b = ns.Sphere(0.3), ns.Sphere(0.3)
    a.move((0.5, 0, 0))
    b.move((-0.5, 0, 0))
    return ns.CombineGeometry("UNION").combine(a, b)


def _geo_torus(ns):
    return ns.Torus(0.55, 0.22)


def _geo_linked_tori(ns):
    a, b = ns.Torus(0.45, 0.1), ns.Torus(0.45, 0.1)
    a.move((-0.25, 0, 0))
    b.rotate(np.pi / 2, (1, 0, 0))
    b.move((0.25, 0, 0))
    return ns.CombineGeometry("UNION").combine(a, b)


def _geo_hollow_sphere(ns):
    s = ns.Sphere(0.55)
    s.onion(0.15)
    return s


def _geo_annulus(ns):
    c = ns.Circle(0.5)
    c.onion(0.15)
    return c


# name -> (numpy field of the grid arrays, geometry builder, grid size, resolution, (b0, b1, b2) or (b0, b1) in 2-D)
ANALYTIC = {
    "sphere": (_sphere, _geo_sphere, (2, 2, 2), (33, 33, 33), (1, 0, 0)),
    "two_spheres": (_two_spheres, _geo_two_spheres, (2, 2, 2), (33, 33, 33), (2, 0, 0)),
    "torus": (lambda X, Y, Z: _torus(X, Y, Z, 0.55, 0.22), _geo_torus, (2, 2, 2), (33, 33, 33), (1, 1, 0)),
    "linked_tori": (_linked_tori, _geo_linked_tori, (2, 2, 2), (41, 41, 41), (2, 2, 0)),
    "hollow_sphere": (_hollow_sphere, _geo_hollow_sphere, (2, 2, 2), (33, 33, 33), (1, 0, 1)),
    "annulus": (_annulus, _geo_annulus, (2, 2), (65, 65), (1, 1)),
}


def analytic(name):
    """-> (numpy field on the shape's grid, (size, resolution), expected Betti numbers)."""
    fn, _, size, resolution, want = ANALYTIC[name]
    return fn(*_grid(size, resolution)), (size, resolution), want


def geometry(name, ns):
    """-> (geometry of the package, grid size, resolution, expected Betti numbers)."""
    _, build, size, resolution, want = ANALYTIC[name]
    return build(ns), size, resolution, want
