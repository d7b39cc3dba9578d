"""Sub-voxel occupancy: the fraction of every grid cell that a geometry covers, and from it the volume (kernels:
csrc/sdfk_occupancy.inc, csrc/sdfk_occdev.h).

    from aegolius_amd import occupancy
    occ = occupancy.from_geometry(geometry, (2, 2, 2), (257, 257, 257), samples=4)
    occ.fraction        # (N,) float32 in [0, 1], generate_grid's layout (z fastest): count / 64, exact
    occ.volume          # float: sum of fraction x cell volume
    occ = occupancy.fractions(geometry, (x, y, z), samples=2, level=0.05)       # any strictly increasing axis tables

No fine grid and no coordinate array are made. A voxel of `hard_binarization` is 0 or 1 by the sign at its centre; here it
is the share of its k^d sub-sample points (k = `samples` per axis: 1, 2, 4 or 8) that lie in the solid.

The definition (one definition: this text, the kernels and tests/occupancy_reference.py), per axis table a (float64,
n >= 2 points), every step in float64 in the order written:

    m_i  = (a_i + a_{i+1}) / 2                                  the mid-points
    lo_i = m_{i-1},  hi_i = m_i                                 the cell of point i
    lo_0 = a_0 - (m_0 - a_0),  hi_{n-1} = a_{n-1} + (a_{n-1} - m_{n-2})         end cells are symmetric about their point
    T[i k + j] = float32(lo_i + ((j + 0.5) / k) (hi_i - lo_i))  the sub-sample coordinates, j = 0 .. k - 1
    hw[i] = max_j |T[i k + j] - float32(a_i)|                   the half-width (float64; handed on as a float32 not below it)

The end cells therefore OVERHANG the box of the grid by half a step on every side: the cells of an n-point axis from -1 to 1
cover [-1 - h / 2, 1 + h / 2], h the step. A geometry that reaches the border of the grid is counted out to there. The
sub-sample tables must be strictly increasing as float32 (else the grid is too fine for float32: ValueError). An axis of one
point (the third axis of a 2-D grid) has the single sample 0.0.

Cell (i0, i1, i2) sits at flat index (i0 n1 + i1) n2 + i2. count = the number of its K = k^d points (T0[i0 k + j0],
T1[i1 k + j1], T2[i2 k + j2]) with f32(point) <= float32(level), f32 the package's float32 field (what create() computes:
a NaN value counts as outside); fraction = count / K as float32, which is exact.

Cells far from the surface are not sampled. With c the grid point as float32 (what create() evaluates), rho =
sqrt(hw0^2 + hw1^2 + hw2^2) and L a Lipschitz bound of the field, a cell is FAR iff

    |f(c) - level| > 1.0001 L rho + L cmag + 1e-6 (1 + |f(c)| + |level|),    cmag = 1e-6 (|cx| + |cy| + |cz| + rho)

(float32; a NaN makes the cell near) and gets 1.0 if f(c) <= level, else 0.0: no point within rho of c can lie on the other
side of the level. Only the thin band of near cells around the surface is sampled, one sub-sample per lane. The rule never
changes a bit of the result (tests/test_gpu_occupancy.py compares with the fine grid evaluated in full).

L is the bound the lowering tracks (`LoweredProgram.lipschitz`, as aegolius_amd.render uses it). Where it is infinite —
twist, bend, repetition cells, sign, nearest instance — NOTHING is skipped: every cell is sampled and near_cells == N.
Unlike sphere tracing that is merely slower, never wrong, so it is not an error. An explicit `lipschitz=` is used as given;
a value below the true bound gives wrong fractions silently, and that is the caller's responsibility (as in render). A
bound of 0 (a constant field) skips every cell whose centre value is not within rounding of the level.

Trees that need a staged evaluation (signed, conv_*, custom_*, Python callables) are refused with
autodiff.UnsupportedOpError, as render refuses them. `config.mode`: MODE_NOCULL samples every cell with the plain
specialised kernel, MODE_INTERPRET uses the interpreter's sample kernel (with skipping), MODE_AUTO starts on the interpreter
kernel while the specialised one builds in the background; all give the same bits.

`volume` (area for a 2-D grid) = sum over the cells of count / K x prod (hi - lo) over the cell's axes. The device reduces
sum_i2 fraction x (hi - lo)_2 per row in float64 in a fixed order (sdfk_field_row_sums); the host multiplies the row sums
by the other axes' widths and adds them with numpy in float64. `inside_samples` is the sum of the counts, added as
integers (per-wave partial sums on the device, their sum on the host), so it does not depend on the order.
"""
import numpy as np

from . import _engine
from ._eval import config
from ._lipschitz import given
from .mesh import _level, _tables
from .render import _program, lower

SAMPLES = (1, 2, 4, 8)


# ---- tables -----------------------------------------------------------------------------------------------------------
def _axes(axes):
    """-> (float64 axis tables as the caller gave them — 2 or 3, a third one only for a 3-D grid —, dims)."""
    tagged = getattr(axes, "grid_axes", None)
    given = tagged if tagged is not None else axes
    if tagged is None and isinstance(axes, np.ndarray) and axes.ndim == 2 and axes.shape[0] == 3:
        _tables(axes, 3)                                       # (raises: an untagged generate_grid array)
    given = [np.asarray(a, dtype=np.float64).ravel() for a in given]
    dims = 2 if len(given) == 2 or (len(given) == 3 and given[2].size == 1 and given[2][0] == 0.0) else 3
    _tables(axes, dims)                                        # mesh's checks: count, >= 2 points, strictly increasing float32
    return given[:dims], dims


def _cells(a):
    """(lo, hi) of the cells of one float64 axis table."""
    m = (a[:-1] + a[1:]) / 2.0
    lo = np.empty_like(a)
    hi = np.empty_like(a)
    lo[1:] = m
    hi[:-1] = m
    lo[0] = a[0] - (m[0] - a[0])
    hi[-1] = a[-1] + (a[-1] - m[-1])
    return lo, hi


def _not_below(x64):
    """float32 values that are not below the float64 ones."""
    x32 = x64.astype(np.float32)
    low = x32.astype(np.float64) < x64
    x32[low] = np.nextafter(x32[low], np.float32(np.inf))
    return x32


def _check_samples(samples):
    if isinstance(samples, bool) or samples not in SAMPLES or int(samples) != samples:
        raise ValueError("samples per axis: 1, 2, 4 or 8; got %r" % (samples,))
    return int(samples)


def _sample_tables(given, k):
    tables, half, width = [], [], []
    for axis, a in enumerate(given):
        lo, hi = _cells(a)
        frac = (np.arange(k, dtype=np.float64) + 0.5) / k
        t = (lo[:, None] + frac[None, :] * (hi - lo)[:, None]).astype(np.float32).ravel()
        if not np.all(t[1:] > t[:-1]):
            raise ValueError("axis %d: its %d sub-samples per cell are not strictly increasing as float32 (the grid is too "
                             "fine for float32)" % (axis, k))
        c = a.astype(np.float32).astype(np.float64)
        hw = np.abs(t.astype(np.float64).reshape(-1, k) - c[:, None]).max(axis=1)
        tables.append(t)
        half.append(_not_below(hw))
        width.append(hi - lo)
    return tables, half, width


def sample_tables(axes, samples):
    """Where the sub-samples are: `axes` as for mesh.isosurface / mesh.contour — three strictly increasing tables, two,
    the three of a 2-D generate_grid (third axis the single 0.0) or a tagged generate_grid array -> (tables, half_widths),
    one float32 array per axis given: T (n k values) and hw (n values) of the module text. A single-point axis has
    T = [0.0] and hw = [0.0]."""
    k = _check_samples(samples)
    given, _ = _axes(axes)
    tables, half, _ = _sample_tables(given, k)
    tagged = getattr(axes, "grid_axes", None)
    if len(tagged if tagged is not None else axes) == 3 and len(given) == 2:
        tables.append(np.zeros(1, dtype=np.float32))
        half.append(np.zeros(1, dtype=np.float32))
    return tables, half


# ---- result -----------------------------------------------------------------------------------------------------------
class Occupancy:
    """Result of fractions() / from_geometry(): `fraction` (N,) float32 host array — a DeviceField with resident=True —,
    `shape` (the grid: 2 or 3 sizes), `samples`, `level`, `inside_samples` (exact int: the sum of the counts),
    `near_cells` (cells that were sampled; N when nothing was skipped), `volume` (float; area for a 2-D grid)."""

    def __init__(self, fraction, shape, samples, level, inside_samples, near_cells, volume):
        self.fraction, self.shape, self.samples, self.level = fraction, tuple(shape), samples, level
        self.inside_samples, self.near_cells, self.volume = inside_samples, near_cells, volume

    def __repr__(self):
        return "Occupancy(%s cells, %d^%d samples, volume %.9g, %d near cells)" % (
            " x ".join(map(str, self.shape)), self.samples, len(self.shape), self.volume, self.near_cells)

    def free(self):
        """Release the device memory of a resident result."""
        if isinstance(self.fraction, _engine.DeviceField):
            self.fraction.free()


# ---- public interface ---------------------------------------------------------------------------------------------------
def _lipschitz(low, lipschitz):
    if lipschitz is None:
        L = float(low.lipschitz)
        if np.isnan(L) or L < 0.0:
            raise ValueError("the lowering's Lipschitz bound is %r" % (L,))
        return L                                                # (inf: nothing is skipped; 0: a constant field)
    return given(lipschitz)


def _lattice(geometry, given, dims, k, lipschitz):
    """What fractions() and moments.moments() do once their arguments are checked, in the order in which things are
    refused: sub-sample tables, lowering, Lipschitz bound, program, GPU -> (program; float32 axis, sub-sample and
    half-width tables, three of each — a 2-D grid gets a single-point third axis —; the cell widths per axis given
    (float64); the grid's shape; the bound as a float32 not below it, or inf)."""
    tables, half, width = _sample_tables(given, k)
    low, _first = lower(geometry)                               # UnsupportedOpError for staged trees
    L = _lipschitz(low, lipschitz)
    prog = _program(low)                                        # UnsupportedOpError for programs that read a field
    _engine.require_gpu()
    ax = [np.ascontiguousarray(a, dtype=np.float32) for a in given]
    shape = tuple(a.size for a in ax)
    if dims == 2:
        ax.append(np.zeros(1, dtype=np.float32))
        tables = tables + [np.zeros(1, dtype=np.float32)]
        half = half + [np.zeros(1, dtype=np.float32)]
    L32 = float(_not_below(np.array([L]))[0]) if np.isfinite(L) else float("inf")
    return prog, ax, tables, half, width, shape, L32


def fractions(geometry, axes, samples=4, level=0.0, lipschitz=None, resident=False, timings=None, _slab_cells=0):
    """Occupancy fractions of `geometry` on the cells of the grid `axes` span (see the module text) -> Occupancy.
    `samples`: k sub-samples per axis (1, 2, 4, 8); `level`: the solid is {f <= level}; `lipschitz`: None = the bound the
    lowering derives — if that is infinite nothing is skipped, which is slower and never wrong — or an upper bound of
    |grad f| of your own: too small a value gives wrong fractions silently. `resident=True` leaves the fractions in HBM
    (a DeviceField; Occupancy.free() releases it). `timings`: a dict that receives device-event milliseconds of
    centre / classify / sample / volume."""
    k = _check_samples(samples)
    lv = _level(level)
    given, dims = _axes(axes)
    prog, ax, tables, half, width, shape, L32 = _lattice(geometry, given, dims, k, lipschitz)
    n = int(np.prod(shape))
    field = _engine.DeviceField(n, config.device)
    try:
        inside, near = prog.occupancy_grid(ax, tables, half, k, lv, L32, field.ptr, slab_cells=_slab_cells,
                                           device=config.device, mode=config.mode, timings=timings)
        timer = _engine.Timer(timings)
        timer.mark("start")
        rows = _engine.field_row_sums(field.ptr, n // shape[-1], shape[-1], width[-1])
        timer.mark("volume")
        timer.finish()
        lead = width[0] if dims == 2 else (width[0][:, None] * width[1][None, :]).ravel()
        volume = float(np.sum(rows * lead))
        out = field if resident else field.numpy()
    except BaseException:
        field.free()
        raise
    if not resident:
        field.free()
    return Occupancy(out, shape, k, lv, inside, near, volume)


def from_geometry(geometry, size, resolution, samples=4, level=0.0, lipschitz=None, resident=False):
    """fractions() on the grid generate_grid(size, resolution) spans (2 or 3 sizes), from its axis tables (grid_axes):
    neither the coordinate array nor a finer grid is made."""
    from .cores.helper_functions import grid_axes
    if len(size) not in (2, 3):
        raise ValueError("from_geometry: size has 2 or 3 entries")
    axes, _ = grid_axes(size, resolution)
    return fractions(geometry, axes[:len(size)], samples, level, lipschitz, resident)
