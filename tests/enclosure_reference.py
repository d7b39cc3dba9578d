"""numpy float64 restatement of the box rules of csrc/sdfk_boxdev.h and of the key arithmetic of csrc/sdfk_enclosure.inc
(test infrastructure: no GPU, no native code).

    elo, ehi, mag = enclose(low, factors, lo, hi, pad_ulps)

runs a LoweredProgram (aegolius_amd._lower) on n boxes at once: the same rules, operation by operation, in float64, with
the padding formula pad(M) = (pad_ulps - 2) * 2^-23 * M evaluated in float64 (two of the pad_ulps are left to the
roundings of the float32 additions, see sdfk_boxdev.h). `mag` is, per box, the largest magnitude M any
rule handed to the padding formula or met as a finite end of a value register: what the tolerance
T = n_instr * pad_ulps * 2^-23 * M of the tests is built from.

Primitives are evaluated at the centre by float64 transcriptions of their sdfk_device.h functions; the ones the test
scenes use are restated (PRIMS, and TABLE_PRIMS for those that read a table), any other raises NotImplementedError.
"""
import numpy as np

from aegolius_amd import _ops

BIG = 3.0e38
PI = float(np.float32(np.pi))                   # the constants of sdfk_boxdev.h / sdfk_device.h, as the kernel has them
TWO_PI = float(np.float32(6.283185307179586))
KEY_BITS = 19


# ---- key arithmetic ----------------------------------------------------------------------------------------------------
def key_fields(key):
    key = int(key)
    m = (1 << KEY_BITS) - 1
    return key >> (3 * KEY_BITS), (key >> (2 * KEY_BITS)) & m, (key >> KEY_BITS) & m, key & m


def make_key(level, ix, iy, iz=0):
    return (level << (3 * KEY_BITS)) | (ix << (2 * KEY_BITS)) | (iy << KEY_BITS) | iz


def children(key, dims=3):
    level, ix, iy, iz = key_fields(key)
    out = []
    for k in range(1 << dims):
        out.append(make_key(level + 1, 2 * ix + (k & 1), 2 * iy + ((k >> 1) & 1), 2 * iz + (k >> 2) if dims == 3 else 0))
    return out


def key_box(key, dlo, dhi):
    """float64 ends of the box of a key in the domain [dlo, dhi] (2 or 3 entries each)."""
    level, *idx = key_fields(key)
    lo, hi = [], []
    scale = 1.0 / float(1 << level)
    for a in range(len(dlo)):
        w = float(dhi[a]) - float(dlo[a])
        lo.append(float(dlo[a]) + w * (idx[a] * scale))
        hi.append(float(dhi[a]) if idx[a] + 1 == (1 << level) else float(dlo[a]) + w * ((idx[a] + 1) * scale))
    return np.array(lo), np.array(hi)


def round_out(lo64, hi64):
    lo64, hi64 = np.asarray(lo64, dtype=np.float64), np.asarray(hi64, dtype=np.float64)
    lo, hi = lo64.astype(np.float32), hi64.astype(np.float32)
    up = lo.astype(np.float64) > lo64
    lo[up] = np.nextafter(lo[up], np.float32(-np.inf))
    dn = hi.astype(np.float64) < hi64
    hi[dn] = np.nextafter(hi[dn], np.float32(np.inf))
    return lo, hi


# ---- point functions (float64 transcriptions of sdfk_device.h) ----------------------------------------------------------
def _len2(x, y):
    return np.sqrt(x * x + y * y)


def _len3(x, y, z):
    return np.sqrt(x * x + y * y + z * z)


def _clip(v, lo, hi):
    return np.minimum(np.maximum(v, lo), hi)


def _mod(a, d):
    return np.mod(a, d)


def _signshift_pt(x, c):
    v = np.abs(x) - c
    return np.where(x < 0, -v, v)


def _finrep1(x, c, d, s, hs):
    v = _signshift_pt(x, c)
    with np.errstate(all="ignore"):
        u = _mod(x - d, s) - hs
    return np.where((x >= -d) & (x <= d), u, v)


def pt_xform(p, P, imm):
    x, y, z = p
    return np.stack([P[0] * x + P[1] * y + P[2] * z - P[9], P[3] * x + P[4] * y + P[5] * z - P[10],
                     P[6] * x + P[7] * y + P[8] * z - P[11]])


def pt_lin3(p, P, imm):
    x, y, z = p
    return np.stack([P[0] * x + P[1] * y + P[2] * z, P[3] * x + P[4] * y + P[5] * z, P[6] * x + P[7] * y + P[8] * z])


def pt_elongate(p, P, imm):
    return np.stack([p[a] - _clip(p[a], -P[a], P[a]) for a in range(3)])


def pt_twist(p, P, imm):
    s, c = np.sin(P[0] * p[2]), np.cos(P[0] * p[2])
    return np.stack([c * p[0] - s * p[1], s * p[0] + c * p[1], p[2]])


def pt_bend(p, P, imm):
    R, c, s = P[0], P[1], P[2]
    x, y, z = p
    yr = y - R
    phi = np.arctan2(x, -yr)
    qx = R * phi
    qy = -R + _len2(x, yr)
    sg = np.sign(x)
    wx, wy = x - P[4] * sg, y - P[5]
    ss = np.where(x >= 0, s, -s)
    rx, ry = c * wx + ss * wy, -ss * wx + c * wy
    rigid = P[3] <= np.abs(qx)
    return np.stack([np.where(rigid, rx + P[3] * sg, qx), np.where(rigid, ry, qy), z])


def pt_rotsym(p, P, imm):
    phi = np.arctan2(p[1], p[0])
    phi = np.where(phi < 0, TWO_PI + phi, phi)
    phi = _mod(phi, P[0]) - P[1]
    r = _len2(p[0], p[1])
    return np.stack([r * np.cos(phi) - P[3], r * np.sin(phi), p[2]])


def pt_lininst(p, P, imm):
    x = p[0]
    v = _signshift_pt(x, P[0])
    if P[7] != 0.0:
        u = _mod(x - P[3], P[4]) - P[5]
        v = np.where((x >= P[1]) & (x <= P[2]), u, v)
    return np.stack([v, p[1], p[2]])


def pt_axrev(p, P, imm):
    m = _len2(p[0], p[2])
    return np.stack([P[0] * m - P[1] * p[1] - P[2], P[1] * m + P[0] * p[1], np.zeros_like(m)])


POINT_OPS = {
    "MOVC": lambda p, P, imm: p,
    "XFORM": pt_xform,
    "XLATE": lambda p, P, imm: np.stack([p[0] - P[0], p[1] - P[1], p[2] - P[2]]),
    "LIN3": pt_lin3,
    "CSCALE": lambda p, P, imm: p * P[0],
    "ELONGATE": pt_elongate,
    "REVOLVE": lambda p, P, imm: np.stack([_len2(p[0], p[2]) - P[0], p[1], np.zeros_like(p[0])]),
    "ROT2D": lambda p, P, imm: np.stack([P[0] * p[0] + P[1] * p[1], -P[1] * p[0] + P[0] * p[1], p[2]]),
    "AXREV": pt_axrev,
    "ZEROZ": lambda p, P, imm: np.stack([p[0], p[1], np.zeros_like(p[0])]),
    "TWIST": pt_twist,
    "BEND": pt_bend,
    "INFREP": lambda p, P, imm: np.stack([_mod(p[a] + P[a], P[3 + a]) - P[a] for a in range(3)]),
    "FINREP": lambda p, P, imm: np.stack([_finrep1(p[a], P[a], P[3 + a], P[6 + a], P[9 + a]) for a in range(3)]),
    "SYMMETRY": lambda p, P, imm: np.stack([np.abs(p[a]) if imm == a else p[a] for a in range(3)]),
    "FOLDX": lambda p, P, imm: np.stack([np.abs(p[0]) - P[0], p[1], p[2]]),
    "ROTSYM": pt_rotsym,
    "LININST": pt_lininst,
}


def _max0(v):
    return np.maximum(v, 0.0)


def _min0(v):
    return np.minimum(v, 0.0)


def pr_cylinder(p, P):
    d0, d1 = _len2(p[0], p[1]) - P[0], np.abs(p[2]) - P[1]
    return _min0(np.maximum(d0, d1)) + _len2(_max0(d0), _max0(d1))


def pr_box(p, P):
    q = [np.abs(p[a]) - P[a] for a in range(3)]
    return _len3(_max0(q[0]), _max0(q[1]), _max0(q[2])) + _min0(np.maximum(q[0], np.maximum(q[1], q[2])))


def pr_cone(p, P):
    q0, q1 = P[0], P[1]
    w0, w1 = _len2(p[0], p[1]), p[2] - P[2]
    t1 = _clip((w0 * q0 + w1 * q1) * P[3], 0.0, 1.0)
    ax, ay = w0 - q0 * t1, w1 - q1 * t1
    t2 = _clip(w0 * P[4], 0.0, 1.0)
    bx, by = w0 - q0 * t2, w1 - q1
    d = np.minimum(ax * ax + ay * ay, bx * bx + by * by)
    s = np.maximum(-(w0 * q1 - w1 * q0), -(w1 - q1))
    return np.sqrt(d) * np.sign(s)


def pr_box2(p, P):
    dx, dy = np.abs(p[0]) - P[0], np.abs(p[1]) - P[1]
    return _len2(_max0(dx), _max0(dy)) + _min0(np.maximum(dx, dy))


def pr_rbox2(p, P):
    x, y = p[0], p[1]
    r = np.full_like(x, P[2])
    r = np.where(x > 0, P[3], r)
    r = np.where(y > 0, P[4], r)
    r = np.where((x < 0) & (y > 0), P[5], r)
    dx, dy = (np.abs(x) - P[0]) + r, (np.abs(y) - P[1]) + r
    return _len2(_max0(dx), _max0(dy)) + (_min0(np.maximum(dx, dy)) - r)


def pr_ngon(p, P):
    if P[10] > 0.0:
        x, y = p[0].copy(), np.abs(p[1])
        for _ in range(int(P[10])):
            yr, xr = P[8] * y - P[9] * x, P[8] * x + P[9] * y
            over = yr >= 0.0
            x, y = np.where(over, xr, x), np.where(over, yr, y)
        qx, qy = x - P[0], y
    else:
        phi = np.arctan2(p[1], p[0])
        phi = np.where(phi < 0, TWO_PI + phi, phi)
        phi = _mod(phi, P[1])
        r = _len2(p[0], p[1])
        qx, qy = np.cos(phi) * r - P[0], np.sin(phi) * r
    h = _clip(qx * P[3] + qy * P[4], 0.0, P[7])
    return _len2(qx - P[3] * h, qy - P[4] * h) * np.sign(qx * P[5] + qy * P[6])


def pr_axis(p, P):
    return (p[0] if P[1] == 0.0 else (p[1] if P[1] == 1.0 else p[2])) - P[0]


PRIMS = {
    "P_AXIS": pr_axis,
    "P_SPHERE": lambda p, P: _len3(p[0], p[1], p[2]) - P[0],
    "P_CYLINDER": pr_cylinder,
    "P_BOX": pr_box,
    "P_TORUS": lambda p, P: _len2(_len2(p[0], p[1]) - P[0], p[2]) - P[1],
    "P_PLANE": lambda p, P: p[0] * P[0] + p[1] * P[1] + p[2] * P[2] - P[3],
    "P_CONE": pr_cone,
    "P_CIRCLE": lambda p, P: _len2(p[0], p[1]) - P[0],
    "P_BOX2": pr_box2,
    "P_RBOX2": pr_rbox2,
    "P_NGON": pr_ngon,
    "P_ZSLAB": lambda p, P: np.abs(p[2]) - P[0],
}


def _seg2_sq(px, py, S):
    pax, pay = px - S[0], py - S[1]
    h = _clip((pax * S[2] + pay * S[3]) * S[4], 0.0, 1.0)
    dx, dy = pax - S[2] * h, pay - S[3] * h
    return dx * dx + dy * dy


def pr_segline2(p, P, T):
    tab = T[int(P[1]):int(P[1]) + 5 * int(P[0])].reshape(-1, 5)
    best = np.full_like(p[0], 1.0e32)
    for S in tab:
        best = np.minimum(best, _seg2_sq(p[0], p[1], S))
    return np.sqrt(best)


def pr_nearest2(p, P, T):
    tab = T[int(P[1]):int(P[1]) + 2 * int(P[0])].reshape(-1, 2)
    best = np.full_like(p[0], 3.0e38)
    for x, y in tab:
        best = np.minimum(best, (p[0] - x) ** 2 + (p[1] - y) ** 2)
    return np.sqrt(best)


PRIMS["P_SEGMENT2"] = lambda p, P: np.sqrt(_seg2_sq(p[0], p[1], P))
TABLE_PRIMS = {"P_SEGLINE2": pr_segline2, "P_NEAREST2": pr_nearest2}      # (p, P, T): T the program's table
SIGN_PRIMS = ("P_POLYSIGN", "P_SHAPESIGN")


def v_sigmoid(v, P):
    with np.errstate(over="ignore"):
        return P[0] * (1.0 / (1.0 + np.exp((v - P[2]) * P[1])))


def v_capexp(v, P):
    with np.errstate(over="ignore"):
        return P[0] * np.minimum(np.exp(v * P[1]), 1.0)


def v_gauss(v, P):
    u = (np.maximum(v, 0.0) if P[2] != 0.0 else v) * P[1]
    return P[0] * np.exp(-4.0 * (u * u))


def v_expflag(v, P):
    if P[0] == 0.0:
        u = (np.maximum(v, 0.0) if P[2] != 0.0 else v) * P[1]
        t = -4.0 * (u * u)
    elif P[0] == 1.0:
        t = v * P[1]
    else:
        t = -((v - P[2]) * P[1])
    return np.where(t >= P[3], P[4], P[5])


def v_smoothrelu(v, P):
    u = v * P[0]
    return (u + np.sqrt(u * u + P[1])) * 0.5


def v_slowstart(v, P):
    u = _max0(v * P[0])
    return np.sqrt(u * u + P[1]) - P[2]


# name -> (function, turning point or None, padded, extra magnitude)
VALUE_OPS = {
    "VSCALE": (lambda v, P: P[0] * v, None, False, lambda a, P: 0.0),
    "VSUBC": (lambda v, P: v - P[0], None, False, lambda a, P: 0.0),
    "VAFFINE": (lambda v, P: P[0] * v - P[1], None, False, lambda a, P: 0.0),
    "VABS": (lambda v, P: np.abs(v), lambda P: 0.0, False, lambda a, P: 0.0),
    "VNEG": (lambda v, P: -v, None, False, lambda a, P: 0.0),
    "VSIGN": (lambda v, P: np.sign(v), None, False, lambda a, P: 0.0),
    "VHARDBIN": (lambda v, P: np.where(v <= P[0], 1.0, 0.0), None, False, lambda a, P: 0.0),
    "VONION": (lambda v, P: np.abs(v) - P[0], lambda P: 0.0, False, lambda a, P: 0.0),
    "VCONCENTRIC": (lambda v, P: np.abs(v - P[0]), lambda P: P[0], False, lambda a, P: 0.0),
    "VSIGMOID": (v_sigmoid, None, True, lambda a, P: abs(P[0])),
    "VCAPEXP": (v_capexp, None, True, lambda a, P: abs(P[0])),
    "VLINFALL": (lambda v, P: _clip(1.0 - v * P[1], 0.0, 1.0) * P[0], None, False, lambda a, P: 0.0),
    "VRELU": (lambda v, P: _max0(v * P[0]), None, False, lambda a, P: 0.0),
    "VSMOOTHRELU": (v_smoothrelu, None, True, lambda a, P: np.maximum(np.abs(a[0]), np.abs(a[1])) * abs(P[0])),
    "VSLOWSTART": (v_slowstart, None, True, lambda a, P: np.maximum(np.abs(a[0]), np.abs(a[1])) * abs(P[0]) + abs(P[2])),
    "VGAUSS": (v_gauss, lambda P: 0.0, True, lambda a, P: abs(P[0])),
    "VEXPFLAG": (v_expflag, lambda P: 0.0, False, lambda a, P: 0.0),
}


def c_smin(a, b, P, power):
    t = _max0(P[0] - np.abs(a - b))
    return np.minimum(a, b) - (t ** power) * P[1]


def c_extrude(a, b, P):
    return _min0(np.maximum(a, b)) + _len2(_max0(a), _max0(b))


# ---- the box machine ----------------------------------------------------------------------------------------------------
class _Run:
    def __init__(self, n, pad_ulps):
        self.eps = (pad_ulps - 2) * 2.0 ** -23        # the explicit part of the padding (sdfk_boxdev.h SDFK_BOX_EPS)
        self.mag = np.zeros(n)

    def pad(self, m):
        m = np.broadcast_to(np.asarray(m, dtype=np.float64), self.mag.shape)
        self.mag = np.maximum(self.mag, np.where(np.isfinite(m), m, self.mag))
        return m * self.eps

    def note(self, *ends):
        for v in ends:
            self.mag = np.maximum(self.mag, np.where(np.isfinite(v), np.abs(v), 0.0))


class Box:
    """Coordinate register: centre c (3, n), half extents e (3, n), radius r (n,)."""

    def __init__(self, c, e, r):
        self.c, self.e, self.r = c, e, r

    def mag(self):
        return np.max(np.abs(self.c) + self.e, axis=0)

    lo = property(lambda self: self.c - self.e)
    hi = property(lambda self: self.c + self.e)


def _rho(r, fac):
    return r * fac if fac <= BIG else np.full_like(r, BIG)


def _sym(R, c, e, rho, m):
    M = np.maximum(m, np.max(np.abs(c) + e, axis=0))
    p = R.pad(M)
    e = e + p
    return Box(c, e, np.minimum(rho + p, _len3(e[0], e[1], e[2]) + p))


def _hull(R, c, lo, hi, rho, m):
    e = _max0(np.maximum(hi - c, c - lo))
    mm = np.maximum(m, np.maximum(np.max(np.abs(lo), axis=0), np.max(np.abs(hi), axis=0)))
    return _sym(R, c, e, rho, mm)


def _fold(lo, hi):
    a, b = np.abs(lo), np.abs(hi)
    return np.where((lo <= 0) & (hi >= 0), 0.0, np.minimum(a, b)), np.maximum(a, b)


def _axpy2(a, xlo, xhi, b, ylo, yhi):
    p, q, s, t = a * xlo, a * xhi, b * ylo, b * yhi
    return np.minimum(p, q) + np.minimum(s, t), np.maximum(p, q) + np.maximum(s, t)


class _Join:
    def __init__(self, n):
        self.lo, self.hi = np.full(n, BIG), np.full(n, -BIG)

    def add(self, lo, hi, cond=True):
        cond = np.broadcast_to(cond, self.lo.shape)
        self.lo = np.where(cond, np.minimum(self.lo, lo), self.lo)
        self.hi = np.where(cond, np.maximum(self.hi, hi), self.hi)


def _hits(lo, hi, at):
    return np.ceil((lo - at) / TWO_PI) <= np.floor((hi - at) / TWO_PI)


def _cossin(lo, hi):
    c0, c1, s0, s1 = np.cos(lo), np.cos(hi), np.sin(lo), np.sin(hi)
    clo, chi, slo, shi = np.minimum(c0, c1), np.maximum(c0, c1), np.minimum(s0, s1), np.maximum(s0, s1)
    chi = np.where(_hits(lo, hi, 0.0), 1.0, chi)
    clo = np.where(_hits(lo, hi, PI), -1.0, clo)
    shi = np.where(_hits(lo, hi, 0.5 * PI), 1.0, shi)
    slo = np.where(_hits(lo, hi, -0.5 * PI), -1.0, slo)
    return clo, chi, slo, shi


def _rmul(rlo, rhi, tlo, thi):
    return np.where(tlo < 0, rhi * tlo, rlo * tlo), np.where(thi > 0, rhi * thi, rlo * thi)


def _polar(R, x, y, d):
    rc = _len2(x, y)
    phic = np.arctan2(y, x)
    with np.errstate(invalid="ignore"):
        w = np.arctan2(d, np.sqrt(np.maximum((rc - d) * (rc + d), 0.0))) + R.pad(np.maximum(np.abs(phic), 1.0))
    w = np.where(d < rc, w, PI)
    return phic, np.minimum(w, PI), _max0(rc - d), rc + d


def _bmod(alo, ahi, d, inv, slop):
    c0, c1 = min(0.0, d), max(0.0, d)
    with np.errstate(all="ignore"):
        q0, q1 = np.floor((alo - slop) * inv), np.floor((ahi + slop) * inv)
        same = (q0 == q1) & (np.abs(q0) < 1.0e30)
        lo = np.where(same, np.maximum(c0, alo - q0 * d - slop), c0)
        hi = np.where(same, np.minimum(c1, ahi - q0 * d + slop), c1)
    return lo, hi


def _signshift(lo, hi, c):
    J = _Join(lo.shape[0])
    J.add(_max0(lo) - c, hi - c, hi >= 0)
    J.add(lo + c, _min0(hi) + c, lo < 0)
    return J.lo, J.hi


def _len2range(cx, ex, cy, ey):
    ax, ay = np.abs(cx), np.abs(cy)
    return _len2(_max0(ax - ex), _max0(ay - ey)), _len2(ax + ex, ay + ey)


def _linear(R, b, c, A, rho, m):
    A = np.abs(np.asarray(A, dtype=np.float64).reshape(3, 3))
    return _sym(R, c, A @ b.e, rho, m)


def b_xform(R, b, P, imm, fac, c):
    A = np.abs(np.asarray(P[:9]).reshape(3, 3))
    m = np.max(A @ np.abs(b.c) + np.abs(np.asarray(P[9:12]))[:, None], axis=0)
    return _linear(R, b, c, P[:9], _rho(b.r, fac), m)


def b_lin3(R, b, P, imm, fac, c):
    A = np.abs(np.asarray(P[:9]).reshape(3, 3))
    return _linear(R, b, c, P[:9], _rho(b.r, fac), np.max(A @ np.abs(b.c), axis=0))


def b_elongate(R, b, P, imm, fac, c):
    return _hull(R, c, pt_elongate(b.lo, P, imm), pt_elongate(b.hi, P, imm), _rho(b.r, fac), b.mag())


def b_revolve(R, b, P, imm, fac, c):
    mlo, mhi = _len2range(b.c[0], b.e[0], b.c[2], b.e[2])
    z = np.zeros_like(mlo)
    return _hull(R, c, np.stack([mlo - P[0], b.lo[1], z]), np.stack([mhi - P[0], b.hi[1], z]), _rho(b.r, fac),
                 np.maximum(b.mag(), np.maximum(mhi, abs(P[0]))))


def b_rot2d(R, b, P, imm, fac, c):
    co, s = abs(P[0]), abs(P[1])
    return _sym(R, c, np.stack([co * b.e[0] + s * b.e[1], s * b.e[0] + co * b.e[1], b.e[2]]), _rho(b.r, fac), b.mag())


def b_axrev(R, b, P, imm, fac, c):
    mlo, mhi = _len2range(b.c[0], b.e[0], b.c[2], b.e[2])
    xlo, xhi = _axpy2(P[0], mlo, mhi, -P[1], b.lo[1], b.hi[1])
    ylo, yhi = _axpy2(P[1], mlo, mhi, P[0], b.lo[1], b.hi[1])
    z = np.zeros_like(mlo)
    return _hull(R, c, np.stack([xlo - P[2], ylo, z]), np.stack([xhi - P[2], yhi, z]), _rho(b.r, fac),
                 np.maximum(b.mag(), mhi + np.abs(b.c[1]) + b.e[1] + abs(P[2])))


def b_zeroz(R, b, P, imm, fac, c):
    e = b.e.copy()
    e[2] = 0.0
    return Box(c, e, b.r)


def b_twist(R, b, P, imm, fac, c):
    k = abs(P[0])
    rc, h, d2 = _len2(b.c[0], b.c[1]), k * b.e[2], np.minimum(_len2(b.e[0], b.e[1]), b.r)
    s, co = np.abs(np.sin(P[0] * b.c[2])), np.abs(np.cos(P[0] * b.c[2]))
    wx = np.minimum(d2, (co + h) * b.e[0] + (s + h) * b.e[1])
    wy = np.minimum(d2, (s + h) * b.e[0] + (co + h) * b.e[1])
    ax, ay = np.minimum(rc * h, rc + np.abs(c[0])), np.minimum(rc * h, rc + np.abs(c[1]))
    rmax = rc + d2
    kr = k * rmax
    turn = np.maximum(1.0, k * (np.abs(b.c[2]) + b.e[2]))
    return _sym(R, c, np.stack([ax + wx, ay + wy, b.e[2]]), b.r * (0.5 * (kr + np.sqrt(kr * kr + 4.0))),
                np.maximum(b.mag(), rmax * turn))


def b_bend(R, b, P, imm, fac, c):
    Rr, cc, s = P[0], P[1], P[2]
    n = b.r.shape[0]
    d2 = np.minimum(_len2(b.e[0], b.e[1]), b.r)
    phic, dl, rlo, rhi = _polar(R, -(b.c[1] - Rr), b.c[0], d2)
    plo, phi = phic - dl, phic + dl
    full = (phi > PI) | (plo < -PI)
    plo, phi = np.where(full, -PI, plo), np.where(full, PI, phi)
    mag = np.maximum(b.mag(), np.maximum(abs(Rr) * PI, rhi) + abs(P[3]) + abs(P[4]) + abs(P[5]))
    slop = R.pad(mag)
    qa, qb = Rr * plo, Rr * phi
    qlo, qhi = np.minimum(qa, qb), np.maximum(qa, qb)
    amin, amax = _fold(qlo, qhi)
    xlo, xhi, ylo, yhi = b.lo[0], b.hi[0], b.lo[1], b.hi[1]
    X, Y = _Join(n), _Join(n)
    arc = amin - slop < P[3]
    cap = abs(P[3]) + slop
    X.add(np.maximum(qlo, -cap), np.minimum(qhi, cap), arc)
    Y.add(rlo - Rr, rhi - Rr, arc)
    past = amax + slop >= P[3]
    w0, w1 = _max0(xlo) - P[4], xhi - P[4]
    l, h = _axpy2(cc, w0, w1, s, ylo - P[5], yhi - P[5])
    X.add(l + P[3], h + P[3], past & (xhi >= 0))
    l, h = _axpy2(-s, w0, w1, cc, ylo - P[5], yhi - P[5])
    Y.add(l, h, past & (xhi >= 0))
    w0, w1 = xlo + P[4], _min0(xhi) + P[4]
    l, h = _axpy2(cc, w0, w1, -s, ylo - P[5], yhi - P[5])
    X.add(l - P[3], h - P[3], past & (xlo < 0))
    l, h = _axpy2(s, w0, w1, cc, ylo - P[5], yhi - P[5])
    Y.add(l, h, past & (xlo < 0))
    zero = (xlo <= 0) & (xhi >= 0) & past
    z = np.zeros(n)
    l, h = _axpy2(0.0, z, z, s, ylo - P[5], yhi - P[5])
    X.add(l, h, zero)
    l, h = _axpy2(0.0, z, z, cc, ylo - P[5], yhi - P[5])
    Y.add(l, h, zero)
    return _hull(R, c, np.stack([X.lo, Y.lo, b.lo[2]]), np.stack([X.hi, Y.hi, b.hi[2]]), np.full(n, BIG), mag)


def b_infrep(R, b, P, imm, fac, c):
    m = b.mag() + max(abs(P[0]), abs(P[1]), abs(P[2]))
    slop = R.pad(m)
    lo, hi = [], []
    for a in range(3):
        l, h = _bmod(b.lo[a] + P[a], b.hi[a] + P[a], P[3 + a], P[6 + a], slop)
        lo.append(l - P[a])
        hi.append(h - P[a])
    return _hull(R, c, np.stack(lo), np.stack(hi), np.full_like(m, BIG), m)


def _bfinrep1(lo, hi, c, d, s, hs, inv_s, slop):
    J = _Join(lo.shape[0])
    ml, mh = np.maximum(lo, -d), np.minimum(hi, d)
    t0, t1 = _bmod(np.minimum(ml, mh) - d, np.maximum(ml, mh) - d, s, inv_s, slop)
    J.add(t0 - hs, t1 - hs, ml <= mh + slop)
    t0, t1 = _signshift(np.maximum(lo, np.minimum(d, hi)), hi, c)
    J.add(t0, t1, hi + slop > d)
    t0, t1 = _signshift(lo, np.minimum(hi, np.maximum(-d, lo)), c)
    J.add(t0, t1, lo - slop < -d)
    return J.lo, J.hi


def b_finrep(R, b, P, imm, fac, c):
    m = b.mag() + max(abs(P[0]), abs(P[1]), abs(P[2])) + max(abs(P[3]), abs(P[4]), abs(P[5]))
    slop = R.pad(m)
    ends = [_bfinrep1(b.lo[a], b.hi[a], P[a], P[3 + a], P[6 + a], P[9 + a], P[12 + a], slop) for a in range(3)]
    return _hull(R, c, np.stack([e[0] for e in ends]), np.stack([e[1] for e in ends]), np.full_like(m, BIG), m)


def b_symmetry(R, b, P, imm, fac, c):
    lo, hi = b.lo.copy(), b.hi.copy()
    lo[imm], hi[imm] = _fold(b.lo[imm], b.hi[imm])
    return _hull(R, c, lo, hi, _rho(b.r, fac), b.mag())


def b_foldx(R, b, P, imm, fac, c):
    lo, hi = b.lo.copy(), b.hi.copy()
    l, h = _fold(b.lo[0], b.hi[0])
    lo[0], hi[0] = l - P[0], h - P[0]
    return _hull(R, c, lo, hi, _rho(b.r, fac), np.maximum(b.mag(), abs(P[0])))


def b_rotsym(R, b, P, imm, fac, c):
    d2 = np.minimum(_len2(b.e[0], b.e[1]), b.r)
    phic, dl, rlo, rhi = _polar(R, b.c[0], b.c[1], d2)
    a = np.where(phic < 0, TWO_PI + phic, phic)
    mag = np.maximum(b.mag(), rhi + abs(P[3])) * 8.0
    slop = R.pad(8.0)
    one = (dl < PI) & (a - dl > slop) & (a + dl < TWO_PI - slop)
    l, h = _bmod(a - dl, a + dl, P[0], P[2], slop)
    tlo = np.where(one, l - P[1], min(0.0, P[0]) - P[1])
    thi = np.where(one, h - P[1], max(0.0, P[0]) - P[1])
    clo, chi, slo, shi = _cossin(tlo, thi)
    lx, hx = _rmul(rlo, rhi, clo, chi)
    ly, hy = _rmul(rlo, rhi, slo, shi)
    return _hull(R, c, np.stack([lx - P[3], ly, b.lo[2]]), np.stack([hx - P[3], hy, b.hi[2]]), np.full_like(mag, BIG), mag)


def b_lininst(R, b, P, imm, fac, c):
    lo, hi = b.lo[0], b.hi[0]
    m = b.mag() + abs(P[0]) + abs(P[3]) + abs(P[5])
    slop = R.pad(m)
    if P[7] != 0.0:
        J = _Join(lo.shape[0])
        ml, mh = np.maximum(lo, P[1]), np.minimum(hi, P[2])
        t0, t1 = _bmod(np.minimum(ml, mh) - P[3], np.maximum(ml, mh) - P[3], P[4], P[6], slop)
        J.add(t0 - P[5], t1 - P[5], ml <= mh + slop)
        t0, t1 = _signshift(np.maximum(lo, np.minimum(P[2], hi)), hi, P[0])
        J.add(t0, t1, hi + slop > P[2])
        t0, t1 = _signshift(lo, np.minimum(hi, np.maximum(P[1], lo)), P[0])
        J.add(t0, t1, lo - slop < P[1])
        l, h = J.lo, J.hi
    else:
        l, h = _signshift(lo, hi, P[0])
    return _hull(R, c, np.stack([l, b.lo[1], b.lo[2]]), np.stack([h, b.hi[1], b.hi[2]]), np.full_like(m, BIG), m)


BOX_OPS = {
    "MOVC": lambda R, b, P, imm, fac, c: b,
    "XFORM": b_xform,
    "XLATE": lambda R, b, P, imm, fac, c: _sym(R, c, b.e, _rho(b.r, fac), np.maximum(b.mag(), max(abs(P[0]), abs(P[1]), abs(P[2])))),
    "LIN3": b_lin3,
    "CSCALE": lambda R, b, P, imm, fac, c: _sym(R, c, abs(P[0]) * b.e, _rho(b.r, fac), 0.0),
    "ELONGATE": b_elongate, "REVOLVE": b_revolve, "ROT2D": b_rot2d, "AXREV": b_axrev, "ZEROZ": b_zeroz, "TWIST": b_twist,
    "BEND": b_bend, "INFREP": b_infrep, "FINREP": b_finrep, "SYMMETRY": b_symmetry, "FOLDX": b_foldx, "ROTSYM": b_rotsym,
    "LININST": b_lininst,
}


def _prim(R, v, b, L):
    n = v.shape[0]
    if not L <= BIG:
        return np.full(n, -np.inf), np.full(n, np.inf)
    w = L * np.minimum(b.r, _len3(b.e[0], b.e[1], b.e[2]))
    p = R.pad(np.max(np.abs(b.c), axis=0) + w + np.abs(v))
    return v - w - p, v + w + p


def _pad2(R, lo, hi, a, b, extra):
    m = np.maximum(np.maximum(np.maximum(np.abs(a[0]), np.abs(a[1])), np.maximum(np.abs(b[0]), np.abs(b[1]))), extra)
    p = R.pad(m)
    return lo - p, hi + p


def _combine(R, name, a, b, P):
    neg = lambda v: (-v[1], -v[0])   # noqa: E731
    if name == "VMUL":
        pr = [a[0] * b[0], a[0] * b[1], a[1] * b[0], a[1] * b[1]]
        return np.minimum.reduce(pr), np.maximum.reduce(pr)
    if name == "VADD":
        return a[0] + b[0], a[1] + b[1]
    if name == "VDIFF":
        return a[0] - b[1], a[1] - b[0]
    if name == "VMIN":
        return np.minimum(a[0], b[0]), np.minimum(a[1], b[1])
    if name == "VMAX":
        return np.maximum(a[0], b[0]), np.maximum(a[1], b[1])
    if name == "VSUBTRACT":
        return np.maximum(a[0], -b[1]), np.maximum(a[1], -b[0])
    if name == "SMIN2":
        return _pad2(R, c_smin(a[0], b[0], P, 2), c_smin(a[1], b[1], P, 2), a, b, abs(P[0]))
    if name == "SMIN3":
        return _pad2(R, c_smin(a[0], b[0], P, 3), c_smin(a[1], b[1], P, 3), a, b, abs(P[0]))
    if name == "SMAX3":
        return _pad2(R, -c_smin(-a[0], -b[0], P, 3), -c_smin(-a[1], -b[1], P, 3), a, b, abs(P[0]))
    if name == "SSUB3":
        return _pad2(R, -c_smin(-a[0], b[1], P, 3), -c_smin(-a[1], b[0], P, 3), a, b, abs(P[0]))
    if name == "BOLTZ":
        return _pad2(R, np.minimum(a[0], b[0]), np.maximum(a[1], b[1]), a, b, 0.0)
    if name == "BOLTZSUB":
        nb = neg(b)
        return _pad2(R, np.minimum(a[0], nb[0]), np.maximum(a[1], nb[1]), a, b, 0.0)
    if name == "EXTRUDE":
        return _pad2(R, c_extrude(a[0], b[0], P), c_extrude(a[1], b[1], P), a, b, 0.0)
    raise NotImplementedError(name)


def _value(R, name, a, P):
    fn, turn, padded, extra = VALUE_OPS[name]
    with np.errstate(all="ignore"):
        f0, f1 = fn(a[0], P), fn(a[1], P)
        lo, hi = np.minimum(f0, f1), np.maximum(f0, f1)
        if padded:
            m = np.maximum(np.maximum(np.abs(a[0]), np.abs(a[1])), np.maximum(np.maximum(np.abs(lo), np.abs(hi)), extra(a, P)))
            p = R.pad(m)
            lo, hi = lo - p, hi + p
        if turn is not None:
            t = turn(P)
            ft = fn(np.full_like(a[0], t), P)
            inside = (a[0] <= t) & (t <= a[1])
            lo, hi = np.where(inside, np.minimum(lo, ft), lo), np.where(inside, np.maximum(hi, ft), hi)
    return lo, hi


def start_box(lo, hi):
    """The coordinate register of boxes [lo, hi] ((3, n) float32 ends), as sdfk_box_start."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    c = 0.5 * lo + 0.5 * hi
    e = np.maximum(hi - c, c - lo)
    return Box(c, e, _len3(e[0], e[1], e[2]))


def enclose(low, factors, lo, hi, pad_ulps):
    """-> (enclosure lo, hi, largest magnitude met), three (n,) float64 arrays."""
    n = np.asarray(lo).shape[1]
    R = _Run(n, pad_ulps)
    start = start_box(lo, hi)
    C, V = {}, {}
    prm = np.asarray(low.params, dtype=np.float64)
    tab = np.asarray(low.tables, dtype=np.float64).ravel()
    for i, (word, off) in enumerate(np.asarray(low.code).reshape(-1, 2)):
        word, off = int(word), int(off)
        info = _ops.OPS[word & 255]
        a, b, c = (word >> 8) & 255, (word >> 16) & 255, word >> 24
        P = [float(x) for x in prm[off:off + max(info.nparams, 0)]]
        fac = float(factors[i])
        with np.errstate(all="ignore"):
            if info.kind == "C_C":
                src = C.get(b, start)
                centre = POINT_OPS[info.name](src.c, P, c)
                C[a] = BOX_OPS[info.name](R, src, P, c, fac, centre)
            elif info.kind == "V_C":
                src = C.get(b, start)
                if info.name in SIGN_PRIMS:
                    V[a] = (np.full(n, -1.0), np.full(n, 1.0))
                elif info.name in TABLE_PRIMS:
                    V[a] = _prim(R, TABLE_PRIMS[info.name](src.c, P, tab), src, fac)
                else:
                    if info.name not in PRIMS:
                        raise NotImplementedError("the restatement has no float64 transcription of %s" % info.name)
                    V[a] = _prim(R, PRIMS[info.name](src.c, P), src, fac)
            elif info.kind == "V_V":
                V[a] = _value(R, info.name, V[b], P)
            else:
                V[a] = _combine(R, info.name, V[b], V[c], P)
        if info.kind != "C_C":
            R.note(*V[a])
    elo, ehi = V[int(low.result_reg)]
    elo = np.where(np.isnan(elo), -np.inf, elo)
    ehi = np.where(np.isnan(ehi), np.inf, ehi)
    return elo, ehi, R.mag


def statuses(elo, ehi, level):
    return np.where(ehi <= level, -1, np.where(elo > level, 1, 0)).astype(np.int8)


def refine(low, factors, dlo, dhi, depth, level, pad_ulps):
    """The octree refinement of aegolius_amd.enclosure on the restatement -> per level (inside, outside, mixed) counts and
    the list of the non-outside keys."""
    dims = len(dlo)
    keys, out = [0], []
    for lev in range(depth + 1):
        if not keys:
            out.append(((0, 0, 0), []))
            continue
        ends = [key_box(k, dlo, dhi) for k in keys]
        lo = np.array([e[0] for e in ends]).T
        hi = np.array([e[1] for e in ends]).T
        lo32, hi32 = round_out(lo, hi)
        if dims == 2:
            z = np.zeros((1, lo32.shape[1]), dtype=np.float32)
            lo32, hi32 = np.concatenate([lo32, z]), np.concatenate([hi32, z])
        elo, ehi, _ = enclose(low, factors, lo32, hi32, pad_ulps)
        st = statuses(elo, ehi, level)
        out.append(((int(np.sum(st < 0)), int(np.sum(st > 0)), int(np.sum(st == 0))), [k for k, s in zip(keys, st) if s <= 0]))
        keys = [c for k, s in zip(keys, st) if s == 0 for c in children(k, dims)]
    return out
