"""Mass properties: exact volume, centroid and inertia of a geometry on the sub-sample lattice of `occupancy` (kernels:
csrc/sdfk_moments.inc, csrc/sdfk_momdev.h).

    from aegolius_amd import moments
    mp = moments.from_geometry(geometry, (2, 2, 2), (257, 257, 257), samples=4, density=7850.0)
    mp.volume, mp.mass, mp.centroid        # float, float, (3,) float64
    mp.inertia                             # (3, 3) float64 about the centroid; mp.inertia_about(point), mp.principal()
    mp.index_moments                       # the ten integers everything above is made from
    mp = moments.moments(geometry, (x, y, z), samples=2, level=0.05)            # any UNIFORM axis tables

No fraction field is made or copied: the device returns integers and the host turns them into physical quantities.

The definition (one definition: this text, the kernels and tests/moments_reference.py). Grid, sub-sample tables T,
"inside" (f32(point) <= float32(level), a NaN value outside), the far rule and L are exactly those of
aegolius_amd/occupancy.py.

On axis a with n_a cells and k sub-samples per cell (k = 1 on the single-point third axis of a 2-D grid) the fine index of
sub-sample j of cell i is g = i k + j, and its ODD LATTICE COORDINATE is u = 2 g + 1, 1 <= u <= 2 n_a k - 1. The integer
moments of the solid are these sums over all inside sub-samples, in this fixed order,

    3-D: M = (N, U0, U1, U2, U00, U01, U02, U11, U12, U22)         ten sums
    2-D: M = (N, U0, U1, U00, U01, U11)                            six sums

of the terms 1, u_a and u_a u_b. On the host they are Python ints of unbounded size. They equal a numpy sum over the fine
field bit for bit, in any mode, slab size or wave order: the device adds integers (64-bit partial sums per wave, none of
which can wrap — the launcher checks — and their sum in 128 bits on the host).

World coordinates exist only for UNIFORM axes: with h = (a[-1] - a[0]) / (n - 1) in float64, every a_i must lie within
1e-6 |h| of a_0 + i h; otherwise ValueError ("... not uniform ..."; `occupancy.fractions` takes such tables). Sample u
then sits at x = lo + u s / 2 with s = h / k and lo = a_0 - h / 2 (the overhanging end cells of `occupancy`), and the solid
is the union of the sub-cells (boxes s_0 x s_1 x s_2) whose sample is inside. From M, with dV = prod s:

    volume     = N dV  (area in 2-D),   mass = density volume
    centroid_a = lo_a + (U_a / N) s_a / 2
    S_ab       = density dV (s_a s_b / 4) (U_ab - U_a U_b / N)   [+ density dV N s_a^2 / 12 if a == b]

the central second moments; the diagonal term is the sub-cell's own second moment, with which a box whose faces lie on
fine-cell boundaries gets its closed-form inertia. N U_ab - U_a U_b is formed in exact integer arithmetic before the single
conversion to float64 (S_ab = density dV s_a s_b (N U_ab - U_a U_b) / (4 N), S_aa = density dV s_a^2 (3 (N U_aa - U_a^2) +
N^2) / (12 N)): a body at x = 1000 does not lose its inertia to cancellation. 3-D: the inertia tensor about the centroid
is I = tr(S) 1 - S. 2-D: S (2 x 2) and polar = tr(S).

An empty solid (N == 0) has volume = mass = 0, a NaN centroid and zero tensors; nothing is raised.

Arguments are checked and refused as `occupancy.fractions` does; trees that need a staged evaluation raise
autodiff.UnsupportedOpError; an infinite Lipschitz bound means that nothing is skipped; `config.mode`: MODE_NOCULL samples
every cell with the plain specialised kernel, MODE_INTERPRET uses the interpreter kernel (with skipping), MODE_AUTO starts
on the interpreter kernel while the specialised one builds; all give the same integers.
"""
import numpy as np

from ._eval import config
from .mesh import _level
from .occupancy import _axes, _check_samples, _lattice

PAIRS_3D = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
PAIRS_2D = ((0, 0), (0, 1), (1, 1))


def _uniform(given):
    """-> (lo, h) per axis, float64 arrays; ValueError unless every table is uniform to 1e-6 of its step."""
    lo, step = [], []
    for axis, a in enumerate(given):
        h = (a[-1] - a[0]) / (a.size - 1)
        if not np.all(np.abs(a - (a[0] + np.arange(a.size) * h)) <= 1e-6 * abs(h)):
            raise ValueError("axis %d is not uniform: world coordinates of the moments exist for uniform axis tables only "
                             "(occupancy.fractions takes non-uniform tables)" % axis)
        lo.append(a[0] - h / 2.0)
        step.append(h)
    return np.array(lo), np.array(step)


def _density(density):
    d = float(density)
    if not np.isfinite(d) or d <= 0.0:
        raise ValueError("density must be positive and finite; got %r" % (density,))
    return d


class MassProperties:
    """Result of moments() / from_geometry(): `dims` (2 or 3), `shape` (the grid), `samples`, `level`, `density`,
    `index_moments` (the tuple M of the module text: Python ints), `inside_samples` (= N), `near_cells` (cells that were
    sampled), `volume` (area in 2-D), `mass`, `centroid` (d,), `second_moments` (d, d), `inertia` (3-D: (3, 3) about the
    centroid) or `polar` (2-D: float), `radius_of_gyration`; inertia_about(point), principal()."""

    def __init__(self, index_moments, lo, step, shape, samples, level, density, near_cells):
        M = tuple(int(v) for v in index_moments)
        d = len(shape)
        if len(M) != (10 if d == 3 else 6):
            raise ValueError("%d-D mass properties take %d integer moments; got %d" % (d, 10 if d == 3 else 6, len(M)))
        self.dims, self.shape, self.samples, self.level, self.density = d, tuple(shape), samples, level, density
        self.index_moments, self.inside_samples, self.near_cells = M, M[0], near_cells
        s = np.asarray(step, dtype=np.float64) / samples
        lo = np.asarray(lo, dtype=np.float64)
        N, U = M[0], M[1:1 + d]
        dV = float(np.prod(s))
        self.volume = N * dV
        self.mass = density * self.volume
        S = np.zeros((d, d))
        if N == 0:
            self.centroid = np.full(d, np.nan)
        else:
            self.centroid = np.array([lo[a] + (U[a] / N) * s[a] / 2.0 for a in range(d)])
            for (a, b), Uab in zip(PAIRS_3D if d == 3 else PAIRS_2D, M[1 + d:]):
                central = N * Uab - U[a] * U[b]                    # exact: Python ints
                if a == b:
                    S[a, a] = density * dV * s[a] * s[a] * ((3 * central + N * N) / (12 * N))
                else:
                    S[a, b] = S[b, a] = density * dV * s[a] * s[b] * (central / (4 * N))
        self.second_moments = S
        if d == 3:
            self.inertia = np.trace(S) * np.eye(3) - S
        else:
            self.polar = float(np.trace(S))

    def __repr__(self):
        return "MassProperties(%s cells, %d^%d samples, volume %.9g, mass %.9g, centroid %s)" % (
            " x ".join(map(str, self.shape)), self.samples, self.dims, self.volume, self.mass, self.centroid)

    def inertia_about(self, point):
        """Parallel-axis theorem: 3-D the inertia tensor about `point`, inertia + mass (|r|^2 1 - r r^T), r = point -
        centroid; 2-D the polar moment about `point`, polar + mass |r|^2. The empty solid gives zeros."""
        p = np.asarray(point, dtype=np.float64)
        if p.shape != (self.dims,):
            raise ValueError("inertia_about: a point of %d coordinates" % self.dims)
        if self.inside_samples == 0:
            return np.zeros((3, 3)) if self.dims == 3 else 0.0
        r = p - self.centroid
        if self.dims == 2:
            return self.polar + self.mass * float(r @ r)
        return self.inertia + self.mass * (float(r @ r) * np.eye(3) - np.outer(r, r))

    def principal(self):
        """-> (principal moments, ascending; their axes as columns): numpy.linalg.eigh of `inertia`, in 2-D of
        `second_moments`."""
        return np.linalg.eigh(self.inertia if self.dims == 3 else self.second_moments)

    @property
    def radius_of_gyration(self):
        """3-D: (3,) sqrt(inertia_aa / mass) about the coordinate axes through the centroid; 2-D: sqrt(polar / mass).
        NaN for the empty solid."""
        if self.inside_samples == 0:
            return np.full(3, np.nan) if self.dims == 3 else float("nan")
        if self.dims == 2:
            return float(np.sqrt(self.polar / self.mass))
        return np.sqrt(np.diag(self.inertia) / self.mass)


def moments(geometry, axes, samples=4, level=0.0, lipschitz=None, density=1.0, timings=None, _slab_cells=0):
    """Mass properties of the solid {f <= level} of `geometry` on the grid the UNIFORM tables `axes` span (see the module
    text) -> MassProperties. `samples`, `level`, `lipschitz` as for occupancy.fractions; `density`: mass per unit volume
    (area in 2-D). `timings`: a dict that receives device-event milliseconds of centre / far / sample."""
    k = _check_samples(samples)
    lv = _level(level)
    rho = _density(density)
    given, dims = _axes(axes)
    lo, step = _uniform(given)
    prog, ax, tables, half, _width, shape, L32 = _lattice(geometry, given, dims, k, lipschitz)
    M, near = prog.moments_grid(ax, tables, half, k, lv, L32, slab_cells=_slab_cells, device=config.device, mode=config.mode,
                                timings=timings)
    if dims == 2:                                               # (the third axis has u = 1: U2 = N, U02 = U0, ...)
        M = (M[0], M[1], M[2], M[4], M[5], M[7])
    return MassProperties(M, lo, step, shape, k, lv, rho, near)


def from_geometry(geometry, size, resolution, samples=4, level=0.0, lipschitz=None, density=1.0):
    """moments() on the grid generate_grid(size, resolution) spans (2 or 3 sizes), from its axis tables (grid_axes)."""
    from .cores.helper_functions import grid_axes
    if len(size) not in (2, 3):
        raise ValueError("from_geometry: size has 2 or 3 entries")
    axes, _ = grid_axes(size, resolution)
    return moments(geometry, axes[:len(size)], samples, level, lipschitz, density)
