// sdfk_boxdev.h — interval (box) rules of the sdfk register machine: every opcode of sdfk_ops.def that has a rule here
// maps an ENCLOSURE of its operand to an enclosure of its result, so that a program run on an axis-aligned box B gives a
// pair [lo, hi] with lo <= f(p) <= hi for every fp32 point p of B, f being what create() computes (the functions of
// sdfk_device.h in fp32), not the real-arithmetic formula.
//
// Registers
//   coordinate register BC : a centre c, half extents e >= 0 and a radius r >= 0. Invariant: the image of the query box
//                            under the coordinate operations so far lies in box(c, e) ∩ ball(c, r). The centre is ALWAYS
//                            the image of the query box's centre: every coordinate rule computes it by calling the
//                            opcode's own sdfk_device.h function, so a primitive is evaluated at exactly the point
//                            create() reaches from the centre of the box. Extents are the centred hull of the image.
//                            The radius is carried because the axis-aligned hull of a rotated box has a longer diagonal
//                            than the box: through rigid maps r stays the query box's half diagonal.
//   value register BV      : [lo, hi].
// Side table F (one float per instruction, from aegolius_amd/_lipschitz.py): the Lipschitz factor of a coordinate
// operation (r is multiplied by it; +inf: r becomes the half diagonal of the new extents, unless the rule knows a local
// factor) and the Lipschitz constant of a primitive.
//
// Primitives have no interval code of their own: the rule calls the primitive at the centre and returns
// f(c) ± L min(r, |e|).
//
// Rounding: the GPU has no cheap directed rounding, so every rule whose arithmetic can round against the enclosure pads
// its result outward; the padding of one rule is at most SDFK_BOX_PAD_ULPS ulps (2^-23 relative) of the largest magnitude
// M it handled. Of these, SDFK_BOX_PAD_ULPS - 2 are added explicitly (SDFK_BOX_EPS): with M the common scale, twice the
// error of the longest chain of sdfk_device.h (the value at a point of the box and the value at the centre err
// independently) — sd_atan2 1.4 ulp, sd_mod's quotient 1.5, sd_sincos < 1.5, v_sqrt_f32 1, a handful of fmas at 0.5 each:
// below 6 — plus the roundings of the rule's own few operations: 2 x 6 + 2 = 14. The other two are what the additions of
// the padding themselves and the radius or extent the rule reads can round by (half an ulp each, to nearest), so that the
// total stays within the constant: contract (b) of DESIGN.md 4.17 is stated with it.
// Rules that only compose monotone correctly-rounded operations (add, multiply, min, max, abs, compare) of the ends are
// sound without padding and are not padded.
#ifndef SDFK_BOXDEV_H
#define SDFK_BOXDEV_H

#include "sdfk_device.h"

#define SDFK_BOX_PAD_ULPS 16
#define SDFK_BOX_EPS ((SDFK_BOX_PAD_ULPS - 2) * 1.1920928955078125e-7f)
#define SDFK_BOX_BIG 3.0e38f
#define SDFK_BOX_PI 3.14159274101257324f          // fp32 pi, rounded up
#define SDFK_BOX_INV_2PI 0.159154943091895336f

struct BC {
    float cx, cy, cz, ex, ey, ez, r;
};
struct BV {
    float lo, hi;
};

SDFK_DEV float bx_pad(float m) { return m * SDFK_BOX_EPS; }
SDFK_DEV float bx_max3(float a, float b, float c) { return sd_max(a, sd_max(b, c)); }
SDFK_DEV float bx_inf() { return __builtin_huge_valf(); }
// NaN by its bits (the build assumes there are none, so x != x folds away)
SDFK_DEV bool bx_isnan(float x) { return (__builtin_bit_cast(unsigned, x) & 0x7fffffffu) > 0x7f800000u; }
SDFK_DEV V3 bc_c(const BC& b) { V3 p = {b.cx, b.cy, b.cz}; return p; }
// largest coordinate magnitude in the box
SDFK_DEV float bc_mag(const BC& b) { return bx_max3(sd_abs(b.cx) + b.ex, sd_abs(b.cy) + b.ey, sd_abs(b.cz) + b.ez); }
// r * factor, or "unknown" for a factor that is not finite
SDFK_DEV float bx_rho(float r, float fac) { return (fac <= SDFK_BOX_BIG) ? r * fac : SDFK_BOX_BIG; }

// new register from the centre's image c, UNPADDED half extents e, the radius bound rho and the other magnitudes m
SDFK_DEV BC bc_sym(V3 c, float ex, float ey, float ez, float rho, float m) {
    const float M = sd_max(m, bx_max3(sd_abs(c.x) + ex, sd_abs(c.y) + ey, sd_abs(c.z) + ez));
    const float p = bx_pad(M);
    BC r;
    r.cx = c.x, r.cy = c.y, r.cz = c.z;
    r.ex = ex + p, r.ey = ey + p, r.ez = ez + p;
    r.r = sd_min(rho + p, sd_len3(r.ex, r.ey, r.ez) + p);
    return r;
}
// the same from per-axis hulls [lo, hi] of the image: extents are the centred hull about c
SDFK_DEV BC bc_hull(V3 c, float lox, float hix, float loy, float hiy, float loz, float hiz, float rho, float m) {
    const float ex = sd_max0(sd_max(hix - c.x, c.x - lox)), ey = sd_max0(sd_max(hiy - c.y, c.y - loy));
    const float ez = sd_max0(sd_max(hiz - c.z, c.z - loz));
    const float mm = sd_max(m, sd_max(bx_max3(sd_abs(lox), sd_abs(loy), sd_abs(loz)), bx_max3(sd_abs(hix), sd_abs(hiy), sd_abs(hiz))));
    return bc_sym(c, ex, ey, ez, rho, mm);
}

// ---- interval helpers ----------------------------------------------------------------------------------------------
// |x| over [lo, hi]
SDFK_DEV void bx_fold(float lo, float hi, float* olo, float* ohi) {
    const float a = sd_abs(lo), b = sd_abs(hi);
    *ohi = sd_max(a, b);
    *olo = (lo <= 0.0f && hi >= 0.0f) ? 0.0f : sd_min(a, b);
}
// a * [xlo, xhi] + b * [ylo, yhi]
SDFK_DEV void bx_axpy2(float a, float xlo, float xhi, float b, float ylo, float yhi, float* lo, float* hi) {
    const float p = a * xlo, q = a * xhi, s = b * ylo, t = b * yhi;
    *lo = sd_min(p, q) + sd_min(s, t);
    *hi = sd_max(p, q) + sd_max(s, t);
}
SDFK_DEV void bx_join(float lo, float hi, float* olo, float* ohi) {
    *olo = sd_min(*olo, lo);
    *ohi = sd_max(*ohi, hi);
}
// cos and sin over [lo, hi]
SDFK_DEV bool bx_hits(float lo, float hi, float at) {      // at + 2 pi k in [lo, hi] for some integer k
    return __builtin_ceilf((lo - at) * SDFK_BOX_INV_2PI) <= __builtin_floorf((hi - at) * SDFK_BOX_INV_2PI);
}
SDFK_DEV void bx_cossin(float lo, float hi, float* clo, float* chi, float* slo, float* shi) {
    float s0, c0, s1, c1;
    sd_sincos(lo, &s0, &c0);
    sd_sincos(hi, &s1, &c1);
    *clo = sd_min(c0, c1), *chi = sd_max(c0, c1), *slo = sd_min(s0, s1), *shi = sd_max(s0, s1);
    if (bx_hits(lo, hi, 0.0f)) *chi = 1.0f;
    if (bx_hits(lo, hi, SDFK_BOX_PI)) *clo = -1.0f;
    if (bx_hits(lo, hi, 0.5f * SDFK_BOX_PI)) *shi = 1.0f;
    if (bx_hits(lo, hi, -0.5f * SDFK_BOX_PI)) *slo = -1.0f;
}
// [rlo, rhi] (>= 0) times [tlo, thi]
SDFK_DEV void bx_rmul(float rlo, float rhi, float tlo, float thi, float* lo, float* hi) {
    *lo = (tlo < 0.0f) ? rhi * tlo : rlo * tlo;
    *hi = (thi > 0.0f) ? rhi * thi : rlo * thi;
}
// polar enclosure of the disc of radius d about (x, y): angle atan2(y, x) ± dl (dl = pi: every angle), radius [rlo, rhi]
SDFK_DEV void bx_polar(float x, float y, float d, float* phic, float* dl, float* rlo, float* rhi) {
    const float rc = sd_len2(x, y);
    *phic = sd_atan2(y, x);
    *rhi = rc + d;
    *rlo = sd_max0(rc - d);
    float w = SDFK_BOX_PI;
    if (d < rc) w = sd_atan2(d, sd_sqrt((rc - d) * (rc + d))) + bx_pad(sd_max(sd_abs(*phic), 1.0f));
    *dl = sd_min(w, SDFK_BOX_PI);
}
// floored modulo of [alo, ahi] by d (inv = 1/d), values the kernel's sd_mod can return: inside one cell the interval is
// shifted; across a cell border (or within `slop` of one) it is the whole cell
SDFK_DEV void bx_mod(float alo, float ahi, float d, float inv, float slop, float* lo, float* hi) {
    const float c0 = sd_min(0.0f, d), c1 = sd_max(0.0f, d);
    const float q0 = __builtin_floorf((alo - slop) * inv), q1 = __builtin_floorf((ahi + slop) * inv);
    *lo = c0, *hi = c1;
    if (q0 == q1 && sd_abs(q0) < 1.0e30f) {
        *lo = sd_max(c0, sd_fma(-q0, d, alo) - slop);
        *hi = sd_min(c1, sd_fma(-q0, d, ahi) + slop);
    }
}
// x - c sign(x) over [lo, hi], the value at x = 0 being -c (what |x| - c, negated for x < 0, gives)
SDFK_DEV void bx_signshift(float lo, float hi, float c, float* olo, float* ohi) {
    float l = SDFK_BOX_BIG, h = -SDFK_BOX_BIG;
    if (hi >= 0.0f) bx_join(sd_max0(lo) - c, hi - c, &l, &h);
    if (lo < 0.0f) bx_join(lo + c, sd_min0(hi) + c, &l, &h);
    *olo = l, *ohi = h;
}

// =============================================================================================
// coordinate -> coordinate   BC f(BC b, P, T, imm, fac)
// =============================================================================================
#define SDFK_BOX_C_C(name) SDFK_DEV BC name(const BC& b, const float* __restrict__ P, const float* __restrict__ T, int imm, float fac)

SDFK_BOX_C_C(box_op_movc) { return b; }

SDFK_BOX_C_C(box_op_xform) {
    const V3 c = op_xform<float>(bc_c(b), P, T, imm);
    const float a0 = sd_abs(P[0]), a1 = sd_abs(P[1]), a2 = sd_abs(P[2]), a3 = sd_abs(P[3]), a4 = sd_abs(P[4]), a5 = sd_abs(P[5]);
    const float a6 = sd_abs(P[6]), a7 = sd_abs(P[7]), a8 = sd_abs(P[8]);
    const float ax = sd_abs(b.cx), ay = sd_abs(b.cy), az = sd_abs(b.cz);
    const float m = bx_max3(a0 * ax + a1 * ay + a2 * az + sd_abs(P[9]), a3 * ax + a4 * ay + a5 * az + sd_abs(P[10]),
                            a6 * ax + a7 * ay + a8 * az + sd_abs(P[11]));
    return bc_sym(c, a0 * b.ex + a1 * b.ey + a2 * b.ez, a3 * b.ex + a4 * b.ey + a5 * b.ez, a6 * b.ex + a7 * b.ey + a8 * b.ez,
                  bx_rho(b.r, fac), m);
}
SDFK_BOX_C_C(box_op_xlate) {
    const V3 c = op_xlate<float>(bc_c(b), P, T, imm);
    return bc_sym(c, b.ex, b.ey, b.ez, bx_rho(b.r, fac), sd_max(bc_mag(b), bx_max3(sd_abs(P[0]), sd_abs(P[1]), sd_abs(P[2]))));
}
SDFK_BOX_C_C(box_op_lin3) {
    const V3 c = op_lin3<float>(bc_c(b), P, T, imm);
    const float a0 = sd_abs(P[0]), a1 = sd_abs(P[1]), a2 = sd_abs(P[2]), a3 = sd_abs(P[3]), a4 = sd_abs(P[4]), a5 = sd_abs(P[5]);
    const float a6 = sd_abs(P[6]), a7 = sd_abs(P[7]), a8 = sd_abs(P[8]);
    const float ax = sd_abs(b.cx), ay = sd_abs(b.cy), az = sd_abs(b.cz);
    const float m = bx_max3(a0 * ax + a1 * ay + a2 * az, a3 * ax + a4 * ay + a5 * az, a6 * ax + a7 * ay + a8 * az);
    return bc_sym(c, a0 * b.ex + a1 * b.ey + a2 * b.ez, a3 * b.ex + a4 * b.ey + a5 * b.ez, a6 * b.ex + a7 * b.ey + a8 * b.ez,
                  bx_rho(b.r, fac), m);
}
SDFK_BOX_C_C(box_op_cscale) {
    const V3 c = op_cscale<float>(bc_c(b), P, T, imm);
    const float k = sd_abs(P[0]);
    return bc_sym(c, k * b.ex, k * b.ey, k * b.ez, bx_rho(b.r, fac), 0.0f);
}
// x - clip(x, -h, h) is monotone: the ends map to the ends
SDFK_BOX_C_C(box_op_elongate) {
    const V3 c = op_elongate<float>(bc_c(b), P, T, imm);
    const V3 l = {b.cx - b.ex, b.cy - b.ey, b.cz - b.ez}, h = {b.cx + b.ex, b.cy + b.ey, b.cz + b.ez};
    const V3 ql = op_elongate<float>(l, P, T, imm), qh = op_elongate<float>(h, P, T, imm);
    return bc_hull(c, ql.x, qh.x, ql.y, qh.y, ql.z, qh.z, bx_rho(b.r, fac), bc_mag(b));
}
// distance range of the rectangle (cx ± ex, cz ± ez) from the origin
SDFK_DEV void bx_len2range(float cx, float ex, float cy, float ey, float* lo, float* hi) {
    const float ax = sd_abs(cx), ay = sd_abs(cy);
    *lo = sd_len2(sd_max0(ax - ex), sd_max0(ay - ey));
    *hi = sd_len2(ax + ex, ay + ey);
}
SDFK_BOX_C_C(box_op_revolve) {
    const V3 c = op_revolve<float>(bc_c(b), P, T, imm);
    float mlo, mhi;
    bx_len2range(b.cx, b.ex, b.cz, b.ez, &mlo, &mhi);
    return bc_hull(c, mlo - P[0], mhi - P[0], b.cy - b.ey, b.cy + b.ey, 0.0f, 0.0f, bx_rho(b.r, fac),
                   sd_max(bc_mag(b), sd_max(mhi, sd_abs(P[0]))));
}
SDFK_BOX_C_C(box_op_rot2d) {
    const V3 c = op_rot2d<float>(bc_c(b), P, T, imm);
    const float co = sd_abs(P[0]), s = sd_abs(P[1]);
    return bc_sym(c, co * b.ex + s * b.ey, s * b.ex + co * b.ey, b.ez, bx_rho(b.r, fac), bc_mag(b));
}
SDFK_BOX_C_C(box_op_axrev) {
    const V3 c = op_axrev<float>(bc_c(b), P, T, imm);
    float mlo, mhi, xlo, xhi, ylo, yhi;
    bx_len2range(b.cx, b.ex, b.cz, b.ez, &mlo, &mhi);
    bx_axpy2(P[0], mlo, mhi, -P[1], b.cy - b.ey, b.cy + b.ey, &xlo, &xhi);
    bx_axpy2(P[1], mlo, mhi, P[0], b.cy - b.ey, b.cy + b.ey, &ylo, &yhi);
    return bc_hull(c, xlo - P[2], xhi - P[2], ylo, yhi, 0.0f, 0.0f, bx_rho(b.r, fac),
                   sd_max(bc_mag(b), mhi + sd_abs(b.cy) + b.ey + sd_abs(P[2])));
}
SDFK_BOX_C_C(box_op_zeroz) {
    const V3 c = op_zeroz<float>(bc_c(b), P, T, imm);
    BC r = b;
    r.cz = c.z, r.ez = 0.0f;
    return r;
}
// the rotation angle P[0] z is bounded by the z interval: about the centre's image, the rotated xy rectangle moves by at
// most (radius of the centre) x (half the angle range) and keeps extents |R(angle)| e. The radius: up to a rotation the
// Jacobian is the shear [[1, s], [0, 1]] between the tangential direction and z, s = |P[0]| x (distance from the axis),
// whose largest singular value is (s + sqrt(s^2 + 4)) / 2 (NOT sqrt(1 + s^2), which bounds only the stretch of the z
// direction itself); s is largest at the largest distance from the axis in the (convex) box ∩ ball
SDFK_BOX_C_C(box_op_twist) {
    const V3 c = op_twist(bc_c(b), P, T, imm);
    const float k = sd_abs(P[0]);
    const float rc = sd_len2(b.cx, b.cy), h = k * b.ez, d2 = sd_min(sd_len2(b.ex, b.ey), b.r);
    float s, co;
    sd_sincos(P[0] * b.cz, &s, &co);
    s = sd_abs(s), co = sd_abs(co);
    const float wx = sd_min(d2, (co + h) * b.ex + (s + h) * b.ey), wy = sd_min(d2, (s + h) * b.ex + (co + h) * b.ey);
    const float ax = sd_min(rc * h, rc + sd_abs(c.x)), ay = sd_min(rc * h, rc + sd_abs(c.y));
    const float rmax = rc + d2, kr = k * rmax;
    const float turn = sd_max(1.0f, k * (sd_abs(b.cz) + b.ez));             // the angle's own rounding scales with it
    return bc_sym(c, ax + wx, ay + wy, b.ez, b.r * (0.5f * (kr + sd_sqrt(sd_fma(kr, kr, 4.0f)))), sd_max(bc_mag(b), rmax * turn));
}
// angle and radius about the bend centre are bounded by bx_polar; the bent arc and the two rigid continuations are joined
SDFK_BOX_C_C(box_op_bend) {
    const V3 c = op_bend(bc_c(b), P, T, imm);
    const float R = P[0], cc = P[1], s = P[2];
    const float d2 = sd_min(sd_len2(b.ex, b.ey), b.r);
    float phic, dl, rlo, rhi;
    bx_polar(-(b.cy - R), b.cx, d2, &phic, &dl, &rlo, &rhi);
    float plo = phic - dl, phi = phic + dl;
    if (phi > SDFK_BOX_PI || plo < -SDFK_BOX_PI) plo = -SDFK_BOX_PI, phi = SDFK_BOX_PI;      // across the cut of atan2
    const float mag = sd_max(bc_mag(b), sd_max(sd_abs(R) * SDFK_BOX_PI, rhi) + sd_abs(P[3]) + sd_abs(P[4]) + sd_abs(P[5]));
    const float slop = bx_pad(mag);
    const float qa = R * plo, qb = R * phi;
    const float qlo = sd_min(qa, qb), qhi = sd_max(qa, qb);
    float amin, amax;
    bx_fold(qlo, qhi, &amin, &amax);
    const float xlo = b.cx - b.ex, xhi = b.cx + b.ex, ylo = b.cy - b.ey, yhi = b.cy + b.ey;
    float lx = SDFK_BOX_BIG, hx = -SDFK_BOX_BIG, ly = SDFK_BOX_BIG, hy = -SDFK_BOX_BIG;
    if (amin - slop < P[3]) {                                   // some point is on the arc: |R phi| < P[3]
        const float cap = sd_abs(P[3]) + slop;
        bx_join(sd_max(qlo, -cap), sd_min(qhi, cap), &lx, &hx);
        bx_join(rlo - R, rhi - R, &ly, &hy);
    }
    if (amax + slop >= P[3]) {                                  // some point is past it
        float l, h;
        if (xhi >= 0.0f) {
            const float w0 = sd_max0(xlo) - P[4], w1 = xhi - P[4];
            bx_axpy2(cc, w0, w1, s, ylo - P[5], yhi - P[5], &l, &h);
            bx_join(l + P[3], h + P[3], &lx, &hx);
            bx_axpy2(-s, w0, w1, cc, ylo - P[5], yhi - P[5], &l, &h);
            bx_join(l, h, &ly, &hy);
        }
        if (xlo < 0.0f) {
            const float w0 = xlo + P[4], w1 = sd_min0(xhi) + P[4];
            bx_axpy2(cc, w0, w1, -s, ylo - P[5], yhi - P[5], &l, &h);
            bx_join(l - P[3], h - P[3], &lx, &hx);
            bx_axpy2(s, w0, w1, cc, ylo - P[5], yhi - P[5], &l, &h);
            bx_join(l, h, &ly, &hy);
        }
        if (xlo <= 0.0f && xhi >= 0.0f) {                       // x = 0 exactly: sign(x) = 0
            bx_axpy2(0.0f, 0.0f, 0.0f, s, ylo - P[5], yhi - P[5], &l, &h);
            bx_join(l, h, &lx, &hx);
            bx_axpy2(0.0f, 0.0f, 0.0f, cc, ylo - P[5], yhi - P[5], &l, &h);
            bx_join(l, h, &ly, &hy);
        }
    }
    return bc_hull(c, lx, hx, ly, hy, b.cz - b.ez, b.cz + b.ez, SDFK_BOX_BIG, mag);
}
SDFK_BOX_C_C(box_op_infrep) {
    const V3 c = op_infrep(bc_c(b), P, T, imm);
    const float m = bc_mag(b) + bx_max3(sd_abs(P[0]), sd_abs(P[1]), sd_abs(P[2]));
    const float slop = bx_pad(m);
    float lx, hx, ly, hy, lz, hz;
    bx_mod(b.cx - b.ex + P[0], b.cx + b.ex + P[0], P[3], P[6], slop, &lx, &hx);
    bx_mod(b.cy - b.ey + P[1], b.cy + b.ey + P[1], P[4], P[7], slop, &ly, &hy);
    bx_mod(b.cz - b.ez + P[2], b.cz + b.ez + P[2], P[5], P[8], slop, &lz, &hz);
    return bc_hull(c, lx - P[0], hx - P[0], ly - P[1], hy - P[1], lz - P[2], hz - P[2], SDFK_BOX_BIG, m);
}
// sd_finrep1 over [lo, hi]: the repeated middle |x| <= d and the two shifted outsides
SDFK_DEV void bx_finrep1(float lo, float hi, float c, float d, float s, float hs, float inv_s, float slop, float* olo, float* ohi) {
    float l = SDFK_BOX_BIG, h = -SDFK_BOX_BIG, t0, t1;
    const float ml = sd_max(lo, -d), mh = sd_min(hi, d);
    if (ml <= mh + slop) {
        bx_mod(sd_min(ml, mh) - d, sd_max(ml, mh) - d, s, inv_s, slop, &t0, &t1);
        bx_join(t0 - hs, t1 - hs, &l, &h);
    }
    if (hi + slop > d) {
        bx_signshift(sd_max(lo, sd_min(d, hi)), hi, c, &t0, &t1);
        bx_join(t0, t1, &l, &h);
    }
    if (lo - slop < -d) {
        bx_signshift(lo, sd_min(hi, sd_max(-d, lo)), c, &t0, &t1);
        bx_join(t0, t1, &l, &h);
    }
    *olo = l, *ohi = h;
}
SDFK_BOX_C_C(box_op_finrep) {
    const V3 c = op_finrep(bc_c(b), P, T, imm);
    const float m = bc_mag(b) + bx_max3(sd_abs(P[0]), sd_abs(P[1]), sd_abs(P[2])) + bx_max3(sd_abs(P[3]), sd_abs(P[4]), sd_abs(P[5]));
    const float slop = bx_pad(m);
    float lx, hx, ly, hy, lz, hz;
    bx_finrep1(b.cx - b.ex, b.cx + b.ex, P[0], P[3], P[6], P[9], P[12], slop, &lx, &hx);
    bx_finrep1(b.cy - b.ey, b.cy + b.ey, P[1], P[4], P[7], P[10], P[13], slop, &ly, &hy);
    bx_finrep1(b.cz - b.ez, b.cz + b.ez, P[2], P[5], P[8], P[11], P[14], slop, &lz, &hz);
    return bc_hull(c, lx, hx, ly, hy, lz, hz, SDFK_BOX_BIG, m);
}
SDFK_BOX_C_C(box_op_symmetry) {
    const V3 c = op_symmetry<float>(bc_c(b), P, T, imm);
    float lx = b.cx - b.ex, hx = b.cx + b.ex, ly = b.cy - b.ey, hy = b.cy + b.ey, lz = b.cz - b.ez, hz = b.cz + b.ez;
    if (imm == 0) bx_fold(lx, hx, &lx, &hx);
    if (imm == 1) bx_fold(ly, hy, &ly, &hy);
    if (imm == 2) bx_fold(lz, hz, &lz, &hz);
    return bc_hull(c, lx, hx, ly, hy, lz, hz, bx_rho(b.r, fac), bc_mag(b));
}
SDFK_BOX_C_C(box_op_foldx) {
    const V3 c = op_foldx<float>(bc_c(b), P, T, imm);
    float lx, hx;
    bx_fold(b.cx - b.ex, b.cx + b.ex, &lx, &hx);
    return bc_hull(c, lx - P[0], hx - P[0], b.cy - b.ey, b.cy + b.ey, b.cz - b.ez, b.cz + b.ez, bx_rho(b.r, fac),
                   sd_max(bc_mag(b), sd_abs(P[0])));
}
// angle (into [0, 2 pi), then modulo the sector) and radius are bounded by bx_polar; across a sector border, or across
// the seam of the angle at 0 = 2 pi, the angle is the whole sector
SDFK_BOX_C_C(box_op_rotsym) {
    const V3 c = op_rotsym(bc_c(b), P, T, imm);
    const float d2 = sd_min(sd_len2(b.ex, b.ey), b.r);
    float phic, dl, rlo, rhi;
    bx_polar(b.cx, b.cy, d2, &phic, &dl, &rlo, &rhi);
    const float a = (phic < 0.0f) ? SDFK_TWO_PI + phic : phic;
    const float mag = sd_max(bc_mag(b), rhi + sd_abs(P[3])) * 8.0f;          // (angles up to 2 pi scale the radius)
    const float slop = bx_pad(8.0f);
    float tlo = sd_min(0.0f, P[0]) - P[1], thi = sd_max(0.0f, P[0]) - P[1];
    if (dl < SDFK_BOX_PI && a - dl > slop && a + dl < SDFK_TWO_PI - slop) {
        float l, h;
        bx_mod(a - dl, a + dl, P[0], P[2], slop, &l, &h);
        tlo = l - P[1], thi = h - P[1];
    }
    float clo, chi, slo, shi, lx, hx, ly, hy;
    bx_cossin(tlo, thi, &clo, &chi, &slo, &shi);
    bx_rmul(rlo, rhi, clo, chi, &lx, &hx);
    bx_rmul(rlo, rhi, slo, shi, &ly, &hy);
    return bc_hull(c, lx - P[3], hx - P[3], ly, hy, b.cz - b.ez, b.cz + b.ez, SDFK_BOX_BIG, mag);
}
SDFK_BOX_C_C(box_op_lininst) {
    const V3 c = op_lininst(bc_c(b), P, T, imm);
    const float lo = b.cx - b.ex, hi = b.cx + b.ex;
    const float m = bc_mag(b) + sd_abs(P[0]) + sd_abs(P[3]) + sd_abs(P[5]);
    const float slop = bx_pad(m);
    float l = SDFK_BOX_BIG, h = -SDFK_BOX_BIG, t0, t1;
    if (P[7] != 0.0f) {
        const float ml = sd_max(lo, P[1]), mh = sd_min(hi, P[2]);
        if (ml <= mh + slop) {
            bx_mod(sd_min(ml, mh) - P[3], sd_max(ml, mh) - P[3], P[4], P[6], slop, &t0, &t1);
            bx_join(t0 - P[5], t1 - P[5], &l, &h);
        }
        if (hi + slop > P[2]) {
            bx_signshift(sd_max(lo, sd_min(P[2], hi)), hi, P[0], &t0, &t1);
            bx_join(t0, t1, &l, &h);
        }
        if (lo - slop < P[1]) {
            bx_signshift(lo, sd_min(hi, sd_max(P[1], lo)), P[0], &t0, &t1);
            bx_join(t0, t1, &l, &h);
        }
    } else {
        bx_signshift(lo, hi, P[0], &l, &h);
    }
    return bc_hull(c, l, h, b.cy - b.ey, b.cy + b.ey, b.cz - b.ez, b.cz + b.ez, SDFK_BOX_BIG, m);
}

// =============================================================================================
// primitives: the value v the opcode's own function gives at the centre, ± L min(r, |e|)
// =============================================================================================
SDFK_DEV BV box_prim(float v, const BC& b, float L) {
    BV r = {-bx_inf(), bx_inf()};
    if (!(L <= SDFK_BOX_BIG)) return r;
    const float w = L * sd_min(b.r, sd_len3(b.ex, b.ey, b.ez));
    const float p = bx_pad(bx_max3(sd_abs(b.cx), sd_abs(b.cy), sd_abs(b.cz)) + w + sd_abs(v));
    r.lo = v - w - p, r.hi = v + w + p;
    return r;
}
// primitives that return a sign: their value range
SDFK_DEV BV box_sign(float, const BC&, float) {
    BV r = {-1.0f, 1.0f};
    return r;
}

// =============================================================================================
// value -> value   BV f(BV a, P)
// =============================================================================================
#define SDFK_BOX_V_V(name) SDFK_DEV BV name(const BV& a, const float* __restrict__ P)
// hull of the values f0, f1 at the ends (a monotone map), padded by the magnitudes met (pad = false: exact)
SDFK_DEV BV bv_ends(float f0, float f1, const BV& a, float extra, bool pad) {
    BV r = {sd_min(f0, f1), sd_max(f0, f1)};
    if (pad) {
        const float p = bx_pad(sd_max(sd_max(sd_abs(a.lo), sd_abs(a.hi)), bx_max3(sd_abs(r.lo), sd_abs(r.hi), extra)));
        r.lo -= p, r.hi += p;
    }
    return r;
}
// the same for a map with one turning point t, whose value ft counts when t is in the interval
SDFK_DEV BV bv_turn(float f0, float f1, float ft, float t, const BV& a, float extra, bool pad) {
    BV r = bv_ends(f0, f1, a, extra, pad);
    if (a.lo <= t && t <= a.hi) r.lo = sd_min(r.lo, ft), r.hi = sd_max(r.hi, ft);
    return r;
}
#define SDFK_BOX_MONO(name, fn, extra, pad) \
    SDFK_BOX_V_V(name) { return bv_ends(fn(a.lo, P), fn(a.hi, P), a, extra, pad); }
#define SDFK_BOX_TURN(name, fn, t, extra, pad) \
    SDFK_BOX_V_V(name) { return bv_turn(fn(a.lo, P), fn(a.hi, P), fn((float)(t), P), (float)(t), a, extra, pad); }

SDFK_BOX_MONO(box_val_scale, val_scale, 0.0f, false)
SDFK_BOX_MONO(box_val_subc, val_subc, 0.0f, false)
SDFK_BOX_MONO(box_val_affine, val_affine, 0.0f, false)
SDFK_BOX_TURN(box_val_abs, val_abs, 0.0f, 0.0f, false)
SDFK_BOX_MONO(box_val_neg, val_neg, 0.0f, false)
SDFK_BOX_MONO(box_val_sign, val_sign, 0.0f, false)                  // the jumps are monotone steps: hull of the ends
SDFK_BOX_MONO(box_val_hardbin, val_hardbin, 0.0f, false)
SDFK_BOX_TURN(box_val_onion, val_onion, 0.0f, 0.0f, false)
SDFK_BOX_TURN(box_val_concentric, val_concentric, P[0], 0.0f, false)
SDFK_BOX_MONO(box_val_sigmoid, val_sigmoid, sd_abs(P[0]), true)
SDFK_BOX_MONO(box_val_capexp, val_capexp, sd_abs(P[0]), true)
SDFK_BOX_MONO(box_val_linfall, val_linfall, 0.0f, false)
SDFK_BOX_MONO(box_val_relu, val_relu, 0.0f, false)
SDFK_BOX_MONO(box_val_smoothrelu, val_smoothrelu, sd_max(sd_abs(a.lo), sd_abs(a.hi)) * sd_abs(P[0]), true)
SDFK_BOX_MONO(box_val_slowstart, val_slowstart, sd_max(sd_abs(a.lo), sd_abs(a.hi)) * sd_abs(P[0]) + sd_abs(P[2]), true)
SDFK_BOX_TURN(box_val_gauss, val_gauss, 0.0f, sd_abs(P[0]), true)
// the exponent is monotone (kinds 1, 2) or peaks at 0 (kind 0): every value taken is taken at an end or at 0
SDFK_BOX_TURN(box_val_expflag, val_expflag, 0.0f, 0.0f, false)

// =============================================================================================
// (value, value) -> value   BV f(BV a, BV b, P)
// =============================================================================================
#define SDFK_BOX_V_VV(name) SDFK_DEV BV name(const BV& a, const BV& b, const float* __restrict__ P)
SDFK_DEV BV bv_pad2(float lo, float hi, const BV& a, const BV& b, float extra) {
    const float m = sd_max(sd_max(sd_max(sd_abs(a.lo), sd_abs(a.hi)), sd_max(sd_abs(b.lo), sd_abs(b.hi))), extra);
    const float p = bx_pad(m);
    BV r = {lo - p, hi + p};
    return r;
}
SDFK_BOX_V_VV(box_cmb_mul) {                                       // interval product (each product is monotone in each factor)
    const float p0 = a.lo * b.lo, p1 = a.lo * b.hi, p2 = a.hi * b.lo, p3 = a.hi * b.hi;
    BV r = {sd_min(sd_min(p0, p1), sd_min(p2, p3)), sd_max(sd_max(p0, p1), sd_max(p2, p3))};
    return r;
}
SDFK_BOX_V_VV(box_cmb_add) { BV r = {a.lo + b.lo, a.hi + b.hi}; return r; }
SDFK_BOX_V_VV(box_cmb_diff) { BV r = {a.lo - b.hi, a.hi - b.lo}; return r; }
SDFK_BOX_V_VV(box_cmb_min) { BV r = {sd_min(a.lo, b.lo), sd_min(a.hi, b.hi)}; return r; }
SDFK_BOX_V_VV(box_cmb_max) { BV r = {sd_max(a.lo, b.lo), sd_max(a.hi, b.hi)}; return r; }
SDFK_BOX_V_VV(box_cmb_subtract) { BV r = {sd_max(a.lo, -b.hi), sd_max(a.hi, -b.lo)}; return r; }
// the polynomial smooth combiners are monotone in both arguments
SDFK_BOX_V_VV(box_cmb_smin2) { return bv_pad2(cmb_smin2(a.lo, b.lo, P), cmb_smin2(a.hi, b.hi, P), a, b, sd_abs(P[0])); }
SDFK_BOX_V_VV(box_cmb_smin3) { return bv_pad2(cmb_smin3(a.lo, b.lo, P), cmb_smin3(a.hi, b.hi, P), a, b, sd_abs(P[0])); }
SDFK_BOX_V_VV(box_cmb_smax3) { return bv_pad2(cmb_smax3(a.lo, b.lo, P), cmb_smax3(a.hi, b.hi, P), a, b, sd_abs(P[0])); }
SDFK_BOX_V_VV(box_cmb_ssub3) { return bv_pad2(cmb_ssub3(a.lo, b.hi, P), cmb_ssub3(a.hi, b.lo, P), a, b, sd_abs(P[0])); }
// a weighted mean of its operands: the hull of their ends
SDFK_BOX_V_VV(box_cmb_boltz) { return bv_pad2(sd_min(a.lo, b.lo), sd_max(a.hi, b.hi), a, b, 0.0f); }
SDFK_BOX_V_VV(box_cmb_boltzsub) { return bv_pad2(sd_min(a.lo, -b.hi), sd_max(a.hi, -b.lo), a, b, 0.0f); }
SDFK_BOX_V_VV(box_cmb_extrude) { return bv_pad2(cmb_extrude(a.lo, b.lo, P), cmb_extrude(a.hi, b.hi, P), a, b, 0.0f); }

// =============================================================================================
// THE table: which opcodes have a box rule. Kinds: C_C a coordinate rule; V_P a primitive through box_prim (FN is the
// sdfk_device.h function itself); V_S a sign primitive (its value range); V_V / V_VV value rules. The kernel's switch,
// the library's refusal (sdfk_program_box_check / sdfk_box_has_rule) and DESIGN.md's list all come from here. Absent:
// CURVEINST, CURVEINSTT (nearest instance), P_BRAID (no Lipschitz constant on record), V_FIELD (staged evaluation).
// =============================================================================================
#define SDFK_BOX_TABLE(X)                                                                                              \
    X(MOVC, C_C, box_op_movc) X(XFORM, C_C, box_op_xform) X(XLATE, C_C, box_op_xlate) X(LIN3, C_C, box_op_lin3)        \
    X(CSCALE, C_C, box_op_cscale) X(ELONGATE, C_C, box_op_elongate) X(REVOLVE, C_C, box_op_revolve)                    \
    X(ROT2D, C_C, box_op_rot2d) X(AXREV, C_C, box_op_axrev) X(ZEROZ, C_C, box_op_zeroz) X(TWIST, C_C, box_op_twist)    \
    X(BEND, C_C, box_op_bend) X(INFREP, C_C, box_op_infrep) X(FINREP, C_C, box_op_finrep)                              \
    X(SYMMETRY, C_C, box_op_symmetry) X(FOLDX, C_C, box_op_foldx) X(ROTSYM, C_C, box_op_rotsym)                        \
    X(LININST, C_C, box_op_lininst)                                                                                    \
    X(P_AXIS, V_P, prim_axis) X(P_SPHERE, V_P, prim_sphere) X(P_CYLINDER, V_P, prim_cylinder) X(P_BOX, V_P, prim_box)  \
    X(P_TORUS, V_P, prim_torus) X(P_CHAINLINK, V_P, prim_chainlink) X(P_ARC3D, V_P, prim_arc3d)                        \
    X(P_PLANE, V_P, prim_plane) X(P_UPLANE, V_P, prim_uplane) X(P_SEGMENT3, V_P, prim_segment3)                        \
    X(P_CONE, V_P, prim_cone) X(P_INFCONE, V_P, prim_infcone) X(P_SOLIDANGLE, V_P, prim_solidangle)                    \
    X(P_TRIANGLE3, V_P, prim_triangle3) X(P_QUAD3, V_P, prim_quad3) X(P_SEGLINE3, V_P, prim_segline3)                  \
    X(P_NEAREST3, V_P, prim_nearest3) X(P_CIRCLE, V_P, prim_circle) X(P_NEUCIRCLE, V_P, prim_neucircle)                \
    X(P_BOX2, V_P, prim_box2) X(P_SEGMENT2, V_P, prim_segment2) X(P_RBOX2, V_P, prim_rbox2)                            \
    X(P_TRIANGLE2, V_P, prim_triangle2) X(P_ARC2, V_P, prim_arc2) X(P_SECTOR, V_P, prim_sector)                        \
    X(P_INFSECTOR, V_P, prim_infsector) X(P_NGON, V_P, prim_ngon) X(P_SEGLINE2, V_P, prim_segline2)                    \
    X(P_NEAREST2, V_P, prim_nearest2) X(P_ZSLAB, V_P, prim_zslab) X(P_NEARTREE, V_P, prim_neartree)                    \
    X(P_POLYSIGN, V_S, prim_polysign) X(P_SHAPESIGN, V_S, prim_shapesign)                                              \
    X(VSCALE, V_V, box_val_scale) X(VSUBC, V_V, box_val_subc) X(VAFFINE, V_V, box_val_affine) X(VABS, V_V, box_val_abs) \
    X(VNEG, V_V, box_val_neg) X(VSIGN, V_V, box_val_sign) X(VONION, V_V, box_val_onion)                                \
    X(VCONCENTRIC, V_V, box_val_concentric) X(VSIGMOID, V_V, box_val_sigmoid) X(VCAPEXP, V_V, box_val_capexp)          \
    X(VHARDBIN, V_V, box_val_hardbin) X(VLINFALL, V_V, box_val_linfall) X(VRELU, V_V, box_val_relu)                    \
    X(VSMOOTHRELU, V_V, box_val_smoothrelu) X(VSLOWSTART, V_V, box_val_slowstart) X(VGAUSS, V_V, box_val_gauss)        \
    X(VEXPFLAG, V_V, box_val_expflag)                                                                                  \
    X(VMUL, V_VV, box_cmb_mul) X(VADD, V_VV, box_cmb_add) X(VDIFF, V_VV, box_cmb_diff) X(VMIN, V_VV, box_cmb_min)      \
    X(VMAX, V_VV, box_cmb_max) X(VSUBTRACT, V_VV, box_cmb_subtract) X(SMIN2, V_VV, box_cmb_smin2)                      \
    X(SMIN3, V_VV, box_cmb_smin3) X(SMAX3, V_VV, box_cmb_smax3) X(SSUB3, V_VV, box_cmb_ssub3)                          \
    X(BOLTZ, V_VV, box_cmb_boltz) X(BOLTZSUB, V_VV, box_cmb_boltzsub) X(EXTRUDE, V_VV, box_cmb_extrude)

#endif  // SDFK_BOXDEV_H
