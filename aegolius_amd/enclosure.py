"""Interval enclosures: guaranteed bounds of a geometry's field over boxes, and what follows from them on day one — where
a geometry is and a rigorous bracket of its volume (kernels: csrc/sdfk_enclosure.inc, rules: csrc/sdfk_boxdev.h).

    from aegolius_amd import enclosure
    lo, hi = enclosure.enclose(geometry, box_lo, box_hi)              # (3, n) or (2, n) box ends -> n enclosures
    status = enclosure.classify(geometry, (4, 4, 4), (64, 64, 64))    # -1 inside, +1 outside, 0 mixed, per box
    blo, bhi, tight = enclosure.bounding_box(geometry, (4, 4, 4))     # hull of {f <= level} in the domain
    v = enclosure.volume_bounds(geometry, (4, 4, 4), depth=8)         # v.lower <= volume <= v.upper

An enclosure of a box B is a pair [lo, hi] with lo <= f(p) <= hi for every float32 point p of B, f being the float32
field create() computes. It comes from running the geometry's program — create()'s own — on boxes instead of points
(DESIGN.md 4.17 has the rules). Unlike the Lipschitz bound of the lowering, which is one number for all of space and
infinite for twist, bend, repetition and sign, an enclosure is a bound per region: these trees are enclosed like any
other. The contract: (a) sound, with tolerance zero, never NaN, an end a rule cannot bound is infinite; (b) for a tree
with a finite Lipschitz bound L never looser than f(c) ± L r (c the centre, r the half diagonal of B) beyond the rules'
padding; (c) shrinking with the box wherever the tree is continuous.

Boxes given in float64 are rounded outward to float32. A domain is either sizes (s0, s1[, s2]) — the box of
generate_grid(size, ...), centred at the origin — or a pair (lo, hi) of 2- or 3-vectors; 2-D domains have z = 0.

Refinement (bounding_box, volume_bounds): the domain is level 0 of an octree (quadtree in 2-D); a box whose enclosure is
entirely <= level is INSIDE, one entirely > level OUTSIDE, neither is refined; a MIXED box is split into its 8 (4)
children, down to `depth`. Box i of 2^l along an axis of the domain [a, b] is
[a + (b - a) (i / 2^l), a + (b - a) ((i + 1) / 2^l)] in float64 as written, the last one ending at b itself, rounded
outward to float32 for the enclosure. What is returned depends on counts and integer coordinates only, never on the order
in which the device lists the children: every run returns the same bits.

Refused: trees that need a staged evaluation and operations without a box rule (curve instancing, Braid, NeuCircle
orders without a Lipschitz constant) raise autodiff.UnsupportedOpError, naming the operation.
"""
import ctypes

import numpy as np

from . import _engine, _lipschitz, _ops
from ._eval import config
from .autodiff import UnsupportedOpError
from .render import _program, lower

MAX_DEPTH = 19                  # bits per coordinate of a box key
MAX_BOXES = 1 << 22             # default bound of the boxes of one refinement level
KEY_BITS = 19
INSIDE, MIXED, OUTSIDE = -1, 0, 1


# ---- keys (host side of the kernel's arithmetic; tests/enclosure_reference.py restates it) ----------------------------
def make_key(level, ix, iy, iz=0):
    return (np.uint64(level) << np.uint64(3 * KEY_BITS)) | (np.uint64(ix) << np.uint64(2 * KEY_BITS)) | \
        (np.uint64(iy) << np.uint64(KEY_BITS)) | np.uint64(iz)


def _cell_ends(lo, hi, i, level):
    """Ends of cells `i` (int array) of 2^level along [lo, hi], float64, operation by operation as the kernel."""
    scale = 1.0 / float(1 << level)
    w = hi - lo
    i = np.asarray(i, dtype=np.float64)
    a = lo + w * (i * scale)
    b = np.where(i + 1 == (1 << level), hi, lo + w * ((i + 1) * scale))
    return a, b


def round_out(lo64, hi64):
    """float32 ends that contain the float64 ones: the nearest float32 at or below lo, at or above hi."""
    lo64, hi64 = np.asarray(lo64, dtype=np.float64), np.asarray(hi64, dtype=np.float64)
    with np.errstate(over="ignore"):
        lo, hi = lo64.astype(np.float32), hi64.astype(np.float32)
    up = lo.astype(np.float64) > lo64
    lo[up] = np.nextafter(lo[up], np.float32(-np.inf))
    dn = hi.astype(np.float64) < hi64
    hi[dn] = np.nextafter(hi[dn], np.float32(np.inf))
    return lo, hi


# ---- arguments ---------------------------------------------------------------------------------------------------------
def _domain(domain):
    """-> (lo (d,), hi (d,)) float64, d = 2 or 3."""
    d = np.asarray(domain, dtype=np.float64)
    if d.ndim == 1 and d.size in (2, 3):
        lo, hi = -d / 2.0, d / 2.0
    elif d.ndim == 2 and d.shape[0] == 2 and d.shape[1] in (2, 3):
        lo, hi = d[0].copy(), d[1].copy()
    else:
        raise ValueError("a domain is 2 or 3 sizes, or a pair (lo, hi) of 2- or 3-vectors; got shape %r" % (d.shape,))
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
        raise ValueError("the domain must be finite")
    if np.any(lo > hi):
        raise ValueError("the domain is inverted: lo %r > hi %r" % (lo.tolist(), hi.tolist()))
    return lo, hi


def _level(level):
    lv = float(np.float32(level))
    if np.isnan(lv):
        raise ValueError("level is NaN")
    return lv


def _depth(depth):
    if isinstance(depth, bool) or int(depth) != depth or not 0 <= int(depth) <= MAX_DEPTH:
        raise ValueError("depth must be an integer from 0 to %d; got %r" % (MAX_DEPTH, depth))
    return int(depth)


def _boxes(lo, hi):
    """(2 or 3, n) box ends -> (3, n) float32 ends rounded outward."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    if lo.shape != hi.shape or lo.ndim != 2 or lo.shape[0] not in (2, 3):
        raise ValueError("box ends are two arrays of shape (3, n) or (2, n); got %r and %r" % (lo.shape, hi.shape))
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
        raise ValueError("box ends must be finite")
    if np.any(lo > hi):
        raise ValueError("inverted box: a lower end above its upper end (box %d)" % int(np.flatnonzero(np.any(lo > hi, axis=0))[0]))
    lo32, hi32 = round_out(lo, hi)
    if not (np.all(np.isfinite(lo32)) and np.all(np.isfinite(hi32))):
        raise ValueError("box ends must be finite as float32")
    if lo.shape[0] == 2:
        z = np.zeros((1, lo.shape[1]), dtype=np.float32)
        lo32, hi32 = np.concatenate([lo32, z]), np.concatenate([hi32, z])
    return np.ascontiguousarray(lo32), np.ascontiguousarray(hi32)


# ---- the program and its side table ------------------------------------------------------------------------------------
def factors(low):
    """The per-instruction side table of a LoweredProgram (float32, never below the float64 value): the Lipschitz factor
    of a coordinate operation and the Lipschitz constant of a primitive from aegolius_amd._lipschitz (inf: none), 0 for
    value operations."""
    out = np.zeros(len(low.code), dtype=np.float64)
    for i, (word, off) in enumerate(np.asarray(low.code).reshape(-1, 2)):
        info = _ops.OPS[int(word) & 255]
        n = max(info.nparams, 0)
        p = low.params[int(off):int(off) + n]
        if info.kind == "C_C":
            out[i] = _lipschitz.factor(_lipschitz.C_C, info.name, p)
        elif info.kind == "V_C":
            out[i] = _lipschitz.factor(_lipschitz.V_C, info.name, p)
    f32 = out.astype(np.float32)
    low_ = f32.astype(np.float64) < out
    f32[low_] = np.nextafter(f32[low_], np.float32(np.inf))
    return f32


SIGN_PRIMS = ("P_POLYSIGN", "P_SHAPESIGN")


class _Enclosed:
    """A geometry ready to be enclosed: its native program and the factor table on the device."""

    def __init__(self, geometry):
        low, _first = lower(geometry)                           # UnsupportedOpError for staged trees
        self.low = low
        self.prog = _program(low)                               # UnsupportedOpError for programs that read a field
        bad = ctypes.c_int(-1)
        rc = _engine.lib().sdfk_program_box_check(self.prog.handle, ctypes.byref(bad))
        if rc == 1:
            name = _ops.OPS[int(low.code[bad.value, 0]) & 255].name
            raise UnsupportedOpError("opcode %s (instruction %d) has no box rule: the geometry cannot be enclosed"
                                     % (name, bad.value))
        if rc == 2:
            raise UnsupportedOpError("program too large for the enclosure kernel (%d coordinate / %d value registers; 16 / 8 "
                                     "at most)" % (low.n_creg, low.n_vreg))
        _engine.check(rc, "sdfk_program_box_check")
        self.factors = factors(low)
        for i, f in enumerate(self.factors):
            info = _ops.OPS[int(low.code[i, 0]) & 255]
            if info.kind == "V_C" and not np.isfinite(f) and info.name not in SIGN_PRIMS:
                raise UnsupportedOpError("opcode %s (instruction %d) has no finite Lipschitz constant with these parameters: "
                                         "it has no box rule" % (info.name, i))
        self.d_factors = None

    def __enter__(self):
        _engine.require_gpu()
        _engine.check(_engine.lib().sdfk_set_device(int(config.device)), "sdfk_set_device")
        self.d_factors = _engine.DeviceBuffer(max(self.factors.nbytes, 4), what="enclosure factors")
        self.d_factors._filled(self.d_factors.upload, self.factors)
        return self

    def __exit__(self, *exc):
        if self.d_factors is not None:
            self.d_factors.free()

    def enclose(self, lo32, hi32):
        n = lo32.shape[1]
        out_lo, out_hi = np.empty(n, dtype=np.float32), np.empty(n, dtype=np.float32)
        if n == 0:
            return out_lo, out_hi
        with _engine.DeviceRows(3, n, what="box lower ends") as d_lo, _engine.DeviceRows(3, n, what="box upper ends") as d_hi, \
                _engine.DeviceBuffer(8 * n, what="enclosures") as d_out:
            d_lo.upload_rows(lo32)
            d_hi.upload_rows(hi32)
            _engine.check(_engine.lib().sdfk_enclose_boxes_device(self.prog.handle, d_lo.at(), d_hi.at(), n, d_lo.stride,
                                                                  self.d_factors.at(), d_out.at(0, 4 * n), d_out.at(4 * n, 4 * n),
                                                                  None), "sdfk_enclose_boxes_device")
            _engine.check(_engine.lib().sdfk_sync(None), "sdfk_sync")
            d_out.download(out_lo, 0)
            d_out.download(out_hi, 4 * n)
        return out_lo, out_hi


# ---- public interface ----------------------------------------------------------------------------------------------------
def box_opcodes():
    """Names of the opcodes with a box rule (the table in csrc/sdfk_boxdev.h)."""
    lib = _engine.lib()
    return [o.name for o in _ops.OPS if lib.sdfk_box_has_rule(o.code)]


def pad_ulps():
    """The padding constant of the rules (csrc/sdfk_boxdev.h SDFK_BOX_PAD_ULPS)."""
    return int(_engine.lib().sdfk_box_pad_ulps())


def enclose(geometry, lo, hi):
    """Enclosures of `geometry` over n boxes: `lo`, `hi` (3, n) or (2, n: z = 0) arrays of lower and upper ends, finite,
    lo <= hi; float64 ends are rounded outward to float32 -> (lo, hi), two (n,) float32 arrays with
    lo[k] <= f(p) <= hi[k] for every float32 point p of box k."""
    lo32, hi32 = _boxes(lo, hi)
    with _Enclosed(geometry) as enc:
        return enc.enclose(lo32, hi32)


def subdivision(size, divisions):
    """The boxes of classify(): the domain cut into divisions[a] equal parts per axis -> (lo, hi) float32 arrays of shape
    (3, n) (z = 0 for a 2-D domain), box (i0, i1, i2) at flat index (i0 d1 + i1) d2 + i2; ends computed in float64 as
    lo_a + (hi_a - lo_a) (i / d_a) (the last one ends at hi_a itself) and rounded outward."""
    dlo, dhi = _domain(size)
    div = [int(d) for d in np.atleast_1d(divisions)]
    if len(div) == 1:
        div = div * dlo.size
    if len(div) != dlo.size or min(div) < 1:
        raise ValueError("divisions: one positive count per axis of the domain; got %r" % (divisions,))
    ends = []
    for a, d in enumerate(div):
        i = np.arange(d, dtype=np.float64)
        lo = dlo[a] + (dhi[a] - dlo[a]) * (i / d)
        hi = np.where(i + 1 == d, dhi[a], dlo[a] + (dhi[a] - dlo[a]) * ((i + 1) / d))
        ends.append((lo, hi))
    grids_lo = np.meshgrid(*[e[0] for e in ends], indexing="ij")
    grids_hi = np.meshgrid(*[e[1] for e in ends], indexing="ij")
    lo = np.stack([g.ravel() for g in grids_lo])
    hi = np.stack([g.ravel() for g in grids_hi])
    lo32, hi32 = _boxes(lo, hi)
    return lo32, hi32, tuple(div)


def statuses(lo, hi, level=0.0):
    """Status of enclosures against a level: -1 where hi <= level (inside), +1 where lo > level (outside), else 0."""
    lv = np.float32(_level(level))
    return np.where(hi <= lv, INSIDE, np.where(lo > lv, OUTSIDE, MIXED)).astype(np.int8)


def classify(geometry, size, divisions, level=0.0):
    """One status per box of the regular subdivision of the domain `size` into `divisions` parts per axis (see
    subdivision()) -> int8 array of shape `divisions`: -1 the box lies in {f <= level}, +1 it lies outside, 0 undecided."""
    _level(level)
    lo32, hi32, div = subdivision(size, divisions)
    elo, ehi = enclose(geometry, lo32[:len(div)], hi32[:len(div)])
    return statuses(elo, ehi, level).reshape(div)


class VolumeBracket:
    """Result of volume_bounds(): `lower` <= volume of {f <= level} in the domain <= `upper` (area for a 2-D domain);
    `inside`, `outside`, `mixed`: boxes per level 0 .. depth (lists of ints); `depth`, `level`."""

    def __init__(self, lower, upper, inside, outside, mixed, depth, level):
        self.lower, self.upper, self.inside, self.outside, self.mixed = lower, upper, inside, outside, mixed
        self.depth, self.level = depth, level

    width = property(lambda self: self.upper - self.lower)

    def __repr__(self):
        return "VolumeBracket(%.9g .. %.9g, depth %d, %d mixed leaves)" % (self.lower, self.upper, self.depth, self.mixed[-1])


def _refine(geometry, domain, depth, level, max_boxes):
    """-> (domain lo, hi, per level: counts (inside, outside, mixed), hull (min ix iy iz, max ix iy iz) or None)."""
    dlo, dhi = _domain(domain)
    depth, lv = _depth(depth), _level(level)
    if isinstance(max_boxes, bool) or int(max_boxes) != max_boxes or int(max_boxes) < 1:
        raise ValueError("max_boxes must be a positive integer; got %r" % (max_boxes,))
    max_boxes = int(max_boxes)
    dims = dlo.size
    nch = 1 << dims
    dom = (ctypes.c_double * 6)(*([float(x) for x in dlo] + [0.0] * (3 - dims) + [float(x) for x in dhi] + [0.0] * (3 - dims)))
    L = _engine.lib()
    levels = []
    with _Enclosed(geometry) as enc, _engine.DeviceBuffer(L.sdfk_enclose_octree_scratch(), what="octree counters") as scratch:
        # two key lists, read and written in turns; the one to be written grows (at least fourfold, the rate at which the
        # mixed boxes of a surface multiply) when a level can need more than it holds. No per-key status is kept: the
        # counts and the hull are all that is read back.
        lists = [_engine.DeviceBuffer(8, what="octree keys"), None]
        try:
            lists[0].upload(np.zeros(1, dtype=np.uint64))
            n = 1
            for lev in range(depth + 1):
                last = lev == depth
                cap = 0 if last else min(nch * n, max_boxes)
                keys, children = lists[lev & 1], None
                if not last:
                    children = lists[1 - (lev & 1)]
                    if children is None or children.nbytes < 8 * cap:
                        held = 0
                        if children is not None:
                            held = children.nbytes
                            children.free()
                            lists[1 - (lev & 1)] = None
                        children = lists[1 - (lev & 1)] = _engine.DeviceBuffer(min(max(8 * cap, 4 * held), 8 * max_boxes),
                                                                               what="octree keys")
                needed, counts, hull = ctypes.c_int64(0), (ctypes.c_int64 * 3)(), (ctypes.c_int * 6)()
                _engine.check(L.sdfk_enclose_octree_device(
                    enc.prog.handle, keys.at(0, 8 * n), n, dom, dims, lv, enc.d_factors.at(), None,
                    children.at(0, 8 * cap) if children is not None else None, cap, ctypes.byref(needed), counts, hull,
                    scratch.at(), None), "sdfk_enclose_octree_device")
                levels.append((tuple(int(c) for c in counts), tuple(int(h) for h in hull) if hull[3] >= 0 else None))
                if not last and needed.value > cap:
                    raise ValueError("the refinement outgrew max_boxes = %d: level %d (reached from level %d) needs %d boxes; "
                                     "raise max_boxes or lower depth" % (max_boxes, lev + 1, lev, needed.value))
                if last or needed.value == 0:
                    break
                n = int(needed.value)
        finally:
            for buf in lists:
                if buf is not None:
                    buf.free()
    while len(levels) < depth + 1:
        levels.append(((0, 0, 0), None))
    return dlo, dhi, levels


def bounding_box(geometry, domain, depth=8, level=0.0, max_boxes=MAX_BOXES):
    """The smallest hull of octree boxes (down to `depth` levels below `domain`) that is guaranteed to contain
    {f <= level} ∩ domain -> (lo, hi, tight): float64 vectors (2 or 3 entries, as the domain), and `tight` = False when
    the hull touches a face of the domain — the domain was then too small to tell where the solid ends. None when every box
    is outside: the domain holds no point of the solid. `max_boxes` (default 2^22): a refinement level with more boxes
    raises ValueError, which names the level and the count."""
    dlo, dhi, levels = _refine(geometry, domain, depth, level, max_boxes)
    lo = np.full(dlo.size, np.inf)
    hi = np.full(dlo.size, -np.inf)
    for lev, (_counts, hull) in enumerate(levels):
        if hull is None:
            continue
        for a in range(dlo.size):
            l, _ = _cell_ends(dlo[a], dhi[a], np.array([hull[a]]), lev)
            _, h = _cell_ends(dlo[a], dhi[a], np.array([hull[3 + a]]), lev)
            lo[a], hi[a] = min(lo[a], float(l[0])), max(hi[a], float(h[0]))
    if not np.all(np.isfinite(lo)):
        return None
    tight = bool(np.all(lo > dlo) and np.all(hi < dhi))
    return lo, hi, tight


def volume_bounds(geometry, domain, depth=8, level=0.0, max_boxes=MAX_BOXES):
    """A rigorous bracket of the volume (2-D: area) of {f <= level} ∩ domain by octree refinement to `depth` ->
    VolumeBracket: lower = sum over the levels of inside[l] x box volume(l), upper = lower + the volume of the mixed
    leaves (those of the last level), in float64 from the integer counts. `max_boxes` as for bounding_box()."""
    dlo, dhi, levels = _refine(geometry, domain, depth, level, max_boxes)
    total = float(np.prod(dhi - dlo))
    dims = dlo.size
    inside = [c[0] for c, _ in levels]
    outside = [c[1] for c, _ in levels]
    mixed = [c[2] for c, _ in levels]
    lower = 0.0
    for lev, k in enumerate(inside):
        lower += k * (total / float(1 << (dims * lev)))
    upper = lower + mixed[-1] * (total / float(1 << (dims * (len(levels) - 1))))
    return VolumeBracket(lower, upper, inside, outside, mixed, len(levels) - 1, _level(level))
