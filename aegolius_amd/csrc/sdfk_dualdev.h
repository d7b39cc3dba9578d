// sdfk_dualdev.h — forward-mode (dual-number) rules of the sdfk register machine: every opcode of sdfk_ops.def that has
// a rule here carries, next to its value, K tangents d/dθ_k of that value (K = 1..4, a compile-time parameter).
//
// Value channel: every rule computes its value by CALLING the sdfk_device.h function of the opcode, unchanged, and
// recomputes the intermediates it needs for the tangents with the same sd_* calls in the same order. The build uses
// -ffp-contract=off, so those intermediates are bit for bit the ones the value took, and so are the branches below:
// the value of a dual program equals the value create() computes for the same program.
//
// Tangent seeds (sdfk_dual.inc): parameter mode — coordinate tangents start at 0, the tangent of parameter j of an
// instruction for channel k is dP[k * ns + poff + j] (the host differentiates the lowering: aegolius_amd/autodiff.py);
// point mode (K = 3) — the input point's tangents are e_x, e_y, e_z and dP is zero: the tangents are ∇_x f.
//
// Conventions at kinks (documented in DESIGN.md §4.10):
//   * min / max / clip / abs / select: the tangent follows the branch the fp32 value computation took; at an exact tie of
//     min(a, b) / max(a, b) it is a's;
//   * abs'(0) = 0, sign' = 0, hard thresholds (VHARDBIN, VSIGN, VEXPFLAG, the sign factors of cones / n-gons /
//     triangles) have tangent 0;
//   * the derivative of a Euclidean norm at 0 is 0, and so is that of atan2 at the origin: tangents are never NaN or Inf
//     where the value is finite;
//   * floored modulo a - q d: q is constant on each piece (recovered from the value as rint((a - r) / d)).
// Tangents are plain fp32 arithmetic (reciprocals by v_rcp_f32); they are not bit-exact with anything and need not be.
#ifndef SDFK_DUALDEV_H
#define SDFK_DUALDEV_H

#include "sdfk_device.h"

#define SDFK_KLOOP _Pragma("unroll") for (int k = 0; k < K; ++k)

template <int K> struct DC {      // coordinate register: point + K tangents of each component
    float x, y, z;
    float dx[K], dy[K], dz[K];
};
template <int K> struct DS {      // value register: value + K tangents
    float v;
    float d[K];
};

// tangent of parameter j of the instruction for channel k
#define SDFK_DQ(k, j) Q[(k) * ns + (j)]

SDFK_DEV float sdd_rcp(float r) { return (r > 0.0f) ? __builtin_amdgcn_rcpf(r) : 0.0f; }   // 1/r, 0 at r = 0 (norms)

template <int K> SDFK_DEV V3 dc_p(const DC<K>& c) { V3 p = {c.x, c.y, c.z}; return p; }

// ---- helpers: value given (bit-exact from the caller), tangents written -----------------------------------------------
// r = sd_len2(x, y)
template <int K> SDFK_DEV void sdd_len2(float x, float y, const float* dx, const float* dy, float r, float* dr) {
    const float inv = sdd_rcp(r);
    SDFK_KLOOP dr[k] = (x * dx[k] + y * dy[k]) * inv;
}
template <int K>
SDFK_DEV void sdd_len3(float x, float y, float z, const float* dx, const float* dy, const float* dz, float r, float* dr) {
    const float inv = sdd_rcp(r);
    SDFK_KLOOP dr[k] = (x * dx[k] + y * dy[k] + z * dz[k]) * inv;
}
// tangent of sd_abs(a)
template <int K> SDFK_DEV void sdd_abs(float a, const float* da, float* out) {
    SDFK_KLOOP out[k] = (a > 0.0f) ? da[k] : ((a < 0.0f) ? -da[k] : 0.0f);
}
// tangent of sd_min(a, b) / sd_max(a, b)
template <int K> SDFK_DEV void sdd_min(float a, float b, const float* da, const float* db, float* out) {
    const bool ta = a <= b;
    SDFK_KLOOP out[k] = ta ? da[k] : db[k];
}
template <int K> SDFK_DEV void sdd_max(float a, float b, const float* da, const float* db, float* out) {
    const bool ta = a >= b;
    SDFK_KLOOP out[k] = ta ? da[k] : db[k];
}
// tangents of max(a, 0) / min(a, 0)
template <int K> SDFK_DEV void sdd_max0(float a, const float* da, float* out) { SDFK_KLOOP out[k] = (a >= 0.0f) ? da[k] : 0.0f; }
template <int K> SDFK_DEV void sdd_min0(float a, const float* da, float* out) { SDFK_KLOOP out[k] = (a <= 0.0f) ? da[k] : 0.0f; }
// tangent of sd_clip(v, lo, hi) = min(max(v, lo), hi), bounds with tangents dlo / dhi
template <int K>
SDFK_DEV void sdd_clip(float v, float lo, float hi, const float* dv, const float* dlo, const float* dhi, float* out) {
    const float m = sd_max(v, lo);
    const bool tv = v >= lo, tm = m <= hi;
    SDFK_KLOOP out[k] = tm ? (tv ? dv[k] : dlo[k]) : dhi[k];
}
// tangent of sd_clip01(v)
template <int K> SDFK_DEV void sdd_clip01(float v, const float* dv, float* out) {
    const float m = sd_max(v, 0.0f);
    const bool tv = v >= 0.0f, tm = m <= 1.0f;
    SDFK_KLOOP out[k] = (tm && tv) ? dv[k] : 0.0f;
}
// tangent of sd_atan2(y, x): (x dy - y dx) / (x^2 + y^2), 0 at the origin
template <int K> SDFK_DEV void sdd_atan2(float y, float x, const float* dy, const float* dx, float* out) {
    const float r2 = sd_fma(x, x, y * y);
    const float inv = sdd_rcp(r2);
    SDFK_KLOOP out[k] = (x * dy[k] - y * dx[k]) * inv;
}
// tangent of r = sd_mod(a, d, inv_d) = a - q d (q constant on the piece)
template <int K>
SDFK_DEV void sdd_mod(float a, float d, float inv_d, float r, const float* da, const float* dd, float* out) {
    const float q = __builtin_rintf((a - r) * inv_d);
    SDFK_KLOOP out[k] = da[k] - q * dd[k];
}

// =============================================================================================
// coordinate -> coordinate   DC f(DC c, P, Q, ns, T, imm)
// =============================================================================================
#define SDFK_DUAL_C_C(name) template <int K> SDFK_DEV DC<K> name(const DC<K>& c, const float* __restrict__ P, \
                                                                  const float* __restrict__ Q, int ns, const float* __restrict__ T, int imm)
template <int K> SDFK_DEV DC<K> dc_with(const DC<K>& c, V3 q) {
    DC<K> r = c;
    r.x = q.x, r.y = q.y, r.z = q.z;
    return r;
}

SDFK_DUAL_C_C(dual_op_movc) { return c; }

SDFK_DUAL_C_C(dual_op_xform) {
    DC<K> r = dc_with(c, op_xform<float>(dc_p(c), P, T, imm));
    SDFK_KLOOP {
        r.dx[k] = P[0] * c.dx[k] + P[1] * c.dy[k] + P[2] * c.dz[k] + SDFK_DQ(k, 0) * c.x + SDFK_DQ(k, 1) * c.y + SDFK_DQ(k, 2) * c.z - SDFK_DQ(k, 9);
        r.dy[k] = P[3] * c.dx[k] + P[4] * c.dy[k] + P[5] * c.dz[k] + SDFK_DQ(k, 3) * c.x + SDFK_DQ(k, 4) * c.y + SDFK_DQ(k, 5) * c.z - SDFK_DQ(k, 10);
        r.dz[k] = P[6] * c.dx[k] + P[7] * c.dy[k] + P[8] * c.dz[k] + SDFK_DQ(k, 6) * c.x + SDFK_DQ(k, 7) * c.y + SDFK_DQ(k, 8) * c.z - SDFK_DQ(k, 11);
    }
    return r;
}
SDFK_DUAL_C_C(dual_op_xlate) {
    DC<K> r = dc_with(c, op_xlate<float>(dc_p(c), P, T, imm));
    SDFK_KLOOP {
        r.dx[k] = c.dx[k] - SDFK_DQ(k, 0);
        r.dy[k] = c.dy[k] - SDFK_DQ(k, 1);
        r.dz[k] = c.dz[k] - SDFK_DQ(k, 2);
    }
    return r;
}
SDFK_DUAL_C_C(dual_op_lin3) {
    DC<K> r = dc_with(c, op_lin3<float>(dc_p(c), P, T, imm));
    SDFK_KLOOP {
        r.dx[k] = P[0] * c.dx[k] + P[1] * c.dy[k] + P[2] * c.dz[k] + SDFK_DQ(k, 0) * c.x + SDFK_DQ(k, 1) * c.y + SDFK_DQ(k, 2) * c.z;
        r.dy[k] = P[3] * c.dx[k] + P[4] * c.dy[k] + P[5] * c.dz[k] + SDFK_DQ(k, 3) * c.x + SDFK_DQ(k, 4) * c.y + SDFK_DQ(k, 5) * c.z;
        r.dz[k] = P[6] * c.dx[k] + P[7] * c.dy[k] + P[8] * c.dz[k] + SDFK_DQ(k, 6) * c.x + SDFK_DQ(k, 7) * c.y + SDFK_DQ(k, 8) * c.z;
    }
    return r;
}
SDFK_DUAL_C_C(dual_op_cscale) {
    DC<K> r = dc_with(c, op_cscale<float>(dc_p(c), P, T, imm));
    SDFK_KLOOP {
        r.dx[k] = P[0] * c.dx[k] + SDFK_DQ(k, 0) * c.x;
        r.dy[k] = P[0] * c.dy[k] + SDFK_DQ(k, 0) * c.y;
        r.dz[k] = P[0] * c.dz[k] + SDFK_DQ(k, 0) * c.z;
    }
    return r;
}
// q = p - clip(p, -e, e) per axis
template <int K> SDFK_DEV void sdd_elong1(float p, float e, const float* dp, const float* Q, int ns, int j, float* out) {
    float dlo[K], dhi[K], dcl[K];
    SDFK_KLOOP dlo[k] = -SDFK_DQ(k, j), dhi[k] = SDFK_DQ(k, j);
    sdd_clip<K>(p, -e, e, dp, dlo, dhi, dcl);
    SDFK_KLOOP out[k] = dp[k] - dcl[k];
}
SDFK_DUAL_C_C(dual_op_elongate) {
    DC<K> r = dc_with(c, op_elongate<float>(dc_p(c), P, T, imm));
    sdd_elong1<K>(c.x, P[0], c.dx, Q, ns, 0, r.dx);
    sdd_elong1<K>(c.y, P[1], c.dy, Q, ns, 1, r.dy);
    sdd_elong1<K>(c.z, P[2], c.dz, Q, ns, 2, r.dz);
    return r;
}
SDFK_DUAL_C_C(dual_op_revolve) {
    DC<K> r = dc_with(c, op_revolve<float>(dc_p(c), P, T, imm));
    float dl[K];
    sdd_len2<K>(c.x, c.z, c.dx, c.dz, sd_len2(c.x, c.z), dl);
    SDFK_KLOOP {
        r.dx[k] = dl[k] - SDFK_DQ(k, 0);
        r.dy[k] = c.dy[k];
        r.dz[k] = 0.0f;
    }
    return r;
}
SDFK_DUAL_C_C(dual_op_rot2d) {
    DC<K> r = dc_with(c, op_rot2d<float>(dc_p(c), P, T, imm));
    SDFK_KLOOP {
        const float dc_ = SDFK_DQ(k, 0), ds_ = SDFK_DQ(k, 1);
        r.dx[k] = P[0] * c.dx[k] + dc_ * c.x + P[1] * c.dy[k] + ds_ * c.y;
        r.dy[k] = -P[1] * c.dx[k] - ds_ * c.x + P[0] * c.dy[k] + dc_ * c.y;
        r.dz[k] = c.dz[k];
    }
    return r;
}
SDFK_DUAL_C_C(dual_op_axrev) {
    DC<K> r = dc_with(c, op_axrev<float>(dc_p(c), P, T, imm));
    const float m = sd_len2(c.x, c.z);
    float dm[K];
    sdd_len2<K>(c.x, c.z, c.dx, c.dz, m, dm);
    SDFK_KLOOP {
        const float dc_ = SDFK_DQ(k, 0), ds_ = SDFK_DQ(k, 1);
        r.dx[k] = P[0] * dm[k] + dc_ * m - P[1] * c.dy[k] - ds_ * c.y - SDFK_DQ(k, 2);
        r.dy[k] = P[1] * dm[k] + ds_ * m + P[0] * c.dy[k] + dc_ * c.y;
        r.dz[k] = 0.0f;
    }
    return r;
}
SDFK_DUAL_C_C(dual_op_zeroz) {
    DC<K> r = dc_with(c, op_zeroz<float>(dc_p(c), P, T, imm));
    SDFK_KLOOP r.dz[k] = 0.0f;
    return r;
}
SDFK_DUAL_C_C(dual_op_twist) {
    DC<K> r = dc_with(c, op_twist(dc_p(c), P, T, imm));
    float s, co;
    sd_sincos(P[0] * c.z, &s, &co);
    SDFK_KLOOP {
        const float dt = SDFK_DQ(k, 0) * c.z + P[0] * c.dz[k];
        const float ds_ = co * dt, dc_ = -s * dt;
        r.dx[k] = dc_ * c.x + co * c.dx[k] - ds_ * c.y - s * c.dy[k];
        r.dy[k] = ds_ * c.x + s * c.dx[k] + dc_ * c.y + co * c.dy[k];
    }
    return r;
}
SDFK_DUAL_C_C(dual_op_bend) {
    DC<K> r = dc_with(c, op_bend(dc_p(c), P, T, imm));
    const float R = P[0], cc = P[1], s = P[2];
    const float yr = c.y - R;
    const float phi = sd_atan2(c.x, -yr);
    const float qx = R * phi;
    const float L = sd_len2(c.x, yr);
    float dyr[K], nyr[K], dphi[K], dl[K];
    SDFK_KLOOP dyr[k] = c.dy[k] - SDFK_DQ(k, 0), nyr[k] = -dyr[k];
    sdd_atan2<K>(c.x, -yr, c.dx, nyr, dphi);
    sdd_len2<K>(c.x, yr, c.dx, dyr, L, dl);
    if (P[3] <= sd_abs(qx)) {
        const float sg = sd_sign(c.x);
        const float wx = c.x - P[4] * sg, wy = c.y - P[5];
        const float sgn_s = (c.x >= 0.0f) ? 1.0f : -1.0f;
        const float ss = (c.x >= 0.0f) ? s : -s;
        SDFK_KLOOP {
            const float dwx = c.dx[k] - SDFK_DQ(k, 4) * sg, dwy = c.dy[k] - SDFK_DQ(k, 5);
            const float dss = sgn_s * SDFK_DQ(k, 2), dcc = SDFK_DQ(k, 1);
            r.dx[k] = dcc * wx + cc * dwx + dss * wy + ss * dwy + SDFK_DQ(k, 3) * sg;
            r.dy[k] = -dss * wx - ss * dwx + dcc * wy + cc * dwy;
        }
    } else {
        SDFK_KLOOP {
            r.dx[k] = SDFK_DQ(k, 0) * phi + R * dphi[k];
            r.dy[k] = -SDFK_DQ(k, 0) + dl[k];
        }
    }
    return r;
}
// sd_mod(p + h, d, 1/d) - h
template <int K>
SDFK_DEV void sdd_infrep1(float p, const float* dp, const float* __restrict__ P, const float* __restrict__ Q, int ns, int i,
                          float* out) {
    const float a = p + P[i];
    const float m = sd_mod(a, P[3 + i], P[6 + i]);
    float da[K], dd[K];
    SDFK_KLOOP da[k] = dp[k] + SDFK_DQ(k, i), dd[k] = SDFK_DQ(k, 3 + i);
    sdd_mod<K>(a, P[3 + i], P[6 + i], m, da, dd, out);
    SDFK_KLOOP out[k] -= SDFK_DQ(k, i);
}
SDFK_DUAL_C_C(dual_op_infrep) {
    DC<K> r = dc_with(c, op_infrep(dc_p(c), P, T, imm));
    sdd_infrep1<K>(c.x, c.dx, P, Q, ns, 0, r.dx);
    sdd_infrep1<K>(c.y, c.dy, P, Q, ns, 1, r.dy);
    sdd_infrep1<K>(c.z, c.dz, P, Q, ns, 2, r.dz);
    return r;
}
// sd_finrep1 with c = P[i], d = P[3+i], s = P[6+i], hs = P[9+i], 1/s = P[12+i]
template <int K>
SDFK_DEV void sdd_finrep1(float x, const float* dx, const float* __restrict__ P, const float* __restrict__ Q, int ns, int i,
                          float* out) {
    const float d = P[3 + i];
    if (x >= -d && x <= d) {
        const float a = x - d;
        const float m = sd_mod(a, P[6 + i], P[12 + i]);
        float da[K], ds[K];
        SDFK_KLOOP da[k] = dx[k] - SDFK_DQ(k, 3 + i), ds[k] = SDFK_DQ(k, 6 + i);
        sdd_mod<K>(a, P[6 + i], P[12 + i], m, da, ds, out);
        SDFK_KLOOP out[k] -= SDFK_DQ(k, 9 + i);
    } else {
        // v = |x| - c, negated for x < 0: x - ... ; abs'(0) = 0
        SDFK_KLOOP out[k] = (x > 0.0f) ? dx[k] - SDFK_DQ(k, i) : ((x < 0.0f) ? dx[k] + SDFK_DQ(k, i) : -SDFK_DQ(k, i));
    }
}
SDFK_DUAL_C_C(dual_op_finrep) {
    DC<K> r = dc_with(c, op_finrep(dc_p(c), P, T, imm));
    sdd_finrep1<K>(c.x, c.dx, P, Q, ns, 0, r.dx);
    sdd_finrep1<K>(c.y, c.dy, P, Q, ns, 1, r.dy);
    sdd_finrep1<K>(c.z, c.dz, P, Q, ns, 2, r.dz);
    return r;
}
SDFK_DUAL_C_C(dual_op_symmetry) {
    DC<K> r = dc_with(c, op_symmetry<float>(dc_p(c), P, T, imm));
    if (imm == 0) sdd_abs<K>(c.x, c.dx, r.dx);
    if (imm == 1) sdd_abs<K>(c.y, c.dy, r.dy);
    if (imm == 2) sdd_abs<K>(c.z, c.dz, r.dz);
    return r;
}
SDFK_DUAL_C_C(dual_op_foldx) {
    DC<K> r = dc_with(c, op_foldx<float>(dc_p(c), P, T, imm));
    sdd_abs<K>(c.x, c.dx, r.dx);
    SDFK_KLOOP r.dx[k] -= SDFK_DQ(k, 0);
    return r;
}
SDFK_DUAL_C_C(dual_op_rotsym) {
    DC<K> r = dc_with(c, op_rotsym(dc_p(c), P, T, imm));
    float phi = sd_atan2(c.y, c.x);
    phi = (phi < 0.0f) ? SDFK_TWO_PI + phi : phi;
    const float m = sd_mod(phi, P[0], P[2]);
    const float ph = m - P[1];
    const float rr = sd_len2(c.x, c.y);
    float s, co;
    sd_sincos(ph, &s, &co);
    float dphi[K], dA[K], dm[K], dr[K];
    sdd_atan2<K>(c.y, c.x, c.dy, c.dx, dphi);
    SDFK_KLOOP dA[k] = SDFK_DQ(k, 0);
    sdd_mod<K>(phi, P[0], P[2], m, dphi, dA, dm);
    sdd_len2<K>(c.x, c.y, c.dx, c.dy, rr, dr);
    SDFK_KLOOP {
        const float dph = dm[k] - SDFK_DQ(k, 1);
        r.dx[k] = dr[k] * co - rr * s * dph - SDFK_DQ(k, 3);
        r.dy[k] = dr[k] * s + rr * co * dph;
    }
    return r;
}
SDFK_DUAL_C_C(dual_op_lininst) {
    DC<K> r = dc_with(c, op_lininst(dc_p(c), P, T, imm));
    const float x = c.x;
    if (P[7] != 0.0f && x >= P[1] && x <= P[2]) {
        const float a = x - P[3];
        const float m = sd_mod(a, P[4], P[6]);
        float da[K], dd[K];
        SDFK_KLOOP da[k] = c.dx[k] - SDFK_DQ(k, 3), dd[k] = SDFK_DQ(k, 4);
        sdd_mod<K>(a, P[4], P[6], m, da, dd, r.dx);
        SDFK_KLOOP r.dx[k] -= SDFK_DQ(k, 5);
    } else {
        SDFK_KLOOP r.dx[k] = (x > 0.0f) ? c.dx[k] - SDFK_DQ(k, 0) : ((x < 0.0f) ? c.dx[k] + SDFK_DQ(k, 0) : -SDFK_DQ(k, 0));
    }
    return r;
}

// =============================================================================================
// primitives: coordinate -> value   DS f(DC c, P, Q, ns, T)
// =============================================================================================
#define SDFK_DUAL_V_C(name) template <int K> SDFK_DEV DS<K> name(const DC<K>& c, const float* __restrict__ P, \
                                                                  const float* __restrict__ Q, int ns, const float* __restrict__ T)

SDFK_DUAL_V_C(dual_prim_axis) {
    DS<K> r;
    r.v = prim_axis<float>(dc_p(c), P, T);
    // the axis as 0 / 1 weights, not as a select of one of three arrays (that would put the register in memory)
    const float wx = (P[1] == 0.0f) ? 1.0f : 0.0f, wy = (P[1] == 1.0f) ? 1.0f : 0.0f, wz = 1.0f - wx - wy;
    SDFK_KLOOP r.d[k] = (wx * c.dx[k] + wy * c.dy[k] + wz * c.dz[k]) - SDFK_DQ(k, 0);
    return r;
}
SDFK_DUAL_V_C(dual_prim_sphere) {
    DS<K> r;
    r.v = prim_sphere<float>(dc_p(c), P, T);
    sdd_len3<K>(c.x, c.y, c.z, c.dx, c.dy, c.dz, sd_len3(c.x, c.y, c.z), r.d);
    SDFK_KLOOP r.d[k] -= SDFK_DQ(k, 0);
    return r;
}
SDFK_DUAL_V_C(dual_prim_circle) {
    DS<K> r;
    r.v = prim_circle<float>(dc_p(c), P, T);
    sdd_len2<K>(c.x, c.y, c.dx, c.dy, sd_len2(c.x, c.y), r.d);
    SDFK_KLOOP r.d[k] -= SDFK_DQ(k, 0);
    return r;
}
SDFK_DUAL_V_C(dual_prim_cylinder) {
    DS<K> r;
    r.v = prim_cylinder<float>(dc_p(c), P, T);
    const float l = sd_len2(c.x, c.y);
    const float d0 = l - P[0], d1 = sd_abs(c.z) - P[1];
    const float m = sd_max(d0, d1), a = sd_max0(d0), b = sd_max0(d1);
    float dd0[K], dd1[K], dm[K], t1[K], da[K], db[K], t2[K];
    sdd_len2<K>(c.x, c.y, c.dx, c.dy, l, dd0);
    sdd_abs<K>(c.z, c.dz, dd1);
    SDFK_KLOOP dd0[k] -= SDFK_DQ(k, 0), dd1[k] -= SDFK_DQ(k, 1);
    sdd_max<K>(d0, d1, dd0, dd1, dm);
    sdd_min0<K>(m, dm, t1);
    sdd_max0<K>(d0, dd0, da);
    sdd_max0<K>(d1, dd1, db);
    sdd_len2<K>(a, b, da, db, sd_len2(a, b), t2);
    SDFK_KLOOP r.d[k] = t1[k] + t2[k];
    return r;
}
SDFK_DUAL_V_C(dual_prim_box) {
    DS<K> r;
    r.v = prim_box<float>(dc_p(c), P, T);
    const float qx = sd_abs(c.x) - P[0], qy = sd_abs(c.y) - P[1], qz = sd_abs(c.z) - P[2];
    const float ax = sd_max0(qx), ay = sd_max0(qy), az = sd_max0(qz);
    float dqx[K], dqy[K], dqz[K], dax[K], day[K], daz[K], t1[K], myz[K], m[K], t2[K];
    sdd_abs<K>(c.x, c.dx, dqx);
    sdd_abs<K>(c.y, c.dy, dqy);
    sdd_abs<K>(c.z, c.dz, dqz);
    SDFK_KLOOP dqx[k] -= SDFK_DQ(k, 0), dqy[k] -= SDFK_DQ(k, 1), dqz[k] -= SDFK_DQ(k, 2);
    sdd_max0<K>(qx, dqx, dax);
    sdd_max0<K>(qy, dqy, day);
    sdd_max0<K>(qz, dqz, daz);
    sdd_len3<K>(ax, ay, az, dax, day, daz, sd_len3(ax, ay, az), t1);
    const float vyz = sd_max(qy, qz);
    sdd_max<K>(qy, qz, dqy, dqz, myz);
    sdd_max<K>(qx, vyz, dqx, myz, m);
    sdd_min0<K>(sd_max(qx, vyz), m, t2);
    SDFK_KLOOP r.d[k] = t1[k] + t2[k];
    return r;
}
// len2(len2(x', y) - R, z) - r
template <int K>
SDFK_DEV void sdd_torus_tail(float x, float y, float z, const float* dx, const float* dy, const float* dz,
                             const float* __restrict__ P, const float* __restrict__ Q, int ns, float* out) {
    const float l = sd_len2(x, y);
    const float a = l - P[0];
    float da[K];
    sdd_len2<K>(x, y, dx, dy, l, da);
    SDFK_KLOOP da[k] -= SDFK_DQ(k, 0);
    sdd_len2<K>(a, z, da, dz, sd_len2(a, z), out);
    SDFK_KLOOP out[k] -= SDFK_DQ(k, 1);
}
SDFK_DUAL_V_C(dual_prim_torus) {
    DS<K> r;
    r.v = prim_torus<float>(dc_p(c), P, T);
    sdd_torus_tail<K>(c.x, c.y, c.z, c.dx, c.dy, c.dz, P, Q, ns, r.d);
    return r;
}
SDFK_DUAL_V_C(dual_prim_chainlink) {
    DS<K> r;
    r.v = prim_chainlink<float>(dc_p(c), P, T);
    const float x = c.x - sd_clip(c.x, -P[2], P[2]);
    float dlo[K], dhi[K], dcl[K], dxx[K];
    SDFK_KLOOP dlo[k] = -SDFK_DQ(k, 2), dhi[k] = SDFK_DQ(k, 2);
    sdd_clip<K>(c.x, -P[2], P[2], c.dx, dlo, dhi, dcl);
    SDFK_KLOOP dxx[k] = c.dx[k] - dcl[k];
    sdd_torus_tail<K>(x, c.y, c.z, dxx, c.dy, c.dz, P, Q, ns, r.d);
    return r;
}
// arcs: x' = c x + s y, y' = |-s x + c y|, psi = clip(atan2(y', x'), 0, hw), (ex, ey) = (x' - R cos psi, y' - R sin psi)
// P[jc], P[js]: cos / sin of the mid angle; P[jr] radius; P[jw] half width
template <int K>
SDFK_DEV void sdd_arc_core(const DC<K>& c, const float* __restrict__ P, const float* __restrict__ Q, int ns, int jr, int jc,
                           int js, int jw, float* ex, float* ey, float* dex, float* dey) {
    float x, y0;
    sd_rotmid(c.x, c.y, P[jc], P[js], &x, &y0);
    const float y = sd_abs(y0);
    const float a = sd_atan2(y, x);
    const float psi = sd_clip(a, 0.0f, P[jw]);
    float s, co;
    sd_sincos(psi, &s, &co);
    *ex = x - P[jr] * co;
    *ey = y - P[jr] * s;
    float dxr[K], dy0[K], dy[K], da[K], zero[K], dw[K], dpsi[K];
    SDFK_KLOOP {
        const float dcm = SDFK_DQ(k, jc), dsm = SDFK_DQ(k, js);
        dxr[k] = dcm * c.x + P[jc] * c.dx[k] + dsm * c.y + P[js] * c.dy[k];
        dy0[k] = -dsm * c.x - P[js] * c.dx[k] + dcm * c.y + P[jc] * c.dy[k];
        zero[k] = 0.0f;
        dw[k] = SDFK_DQ(k, jw);
    }
    sdd_abs<K>(y0, dy0, dy);
    sdd_atan2<K>(y, x, dy, dxr, da);
    sdd_clip<K>(a, 0.0f, P[jw], da, zero, dw, dpsi);
    SDFK_KLOOP {
        const float dR = SDFK_DQ(k, jr);
        dex[k] = dxr[k] - dR * co + P[jr] * s * dpsi[k];
        dey[k] = dy[k] - dR * s - P[jr] * co * dpsi[k];
    }
}
SDFK_DUAL_V_C(dual_prim_arc3d) {
    DS<K> r;
    r.v = prim_arc3d(dc_p(c), P, T);
    float ex, ey, dex[K], dey[K];
    sdd_arc_core<K>(c, P, Q, ns, 0, 2, 3, 4, &ex, &ey, dex, dey);
    sdd_len3<K>(ex, ey, c.z, dex, dey, c.dz, sd_len3(ex, ey, c.z), r.d);
    SDFK_KLOOP r.d[k] -= SDFK_DQ(k, 1);
    return r;
}
SDFK_DUAL_V_C(dual_prim_arc2) {
    DS<K> r;
    r.v = prim_arc2(dc_p(c), P, T);
    float ex, ey, dex[K], dey[K];
    sdd_arc_core<K>(c, P, Q, ns, 0, 1, 2, 3, &ex, &ey, dex, dey);
    sdd_len2<K>(ex, ey, dex, dey, sd_len2(ex, ey), r.d);
    return r;
}
template <int K> SDFK_DEV void sdd_dot3p(const DC<K>& c, const float* __restrict__ P, const float* __restrict__ Q, int ns, float* out) {
    SDFK_KLOOP out[k] = P[0] * c.dx[k] + P[1] * c.dy[k] + P[2] * c.dz[k] + SDFK_DQ(k, 0) * c.x + SDFK_DQ(k, 1) * c.y +
                        SDFK_DQ(k, 2) * c.z;
}
SDFK_DUAL_V_C(dual_prim_plane) {
    DS<K> r;
    r.v = prim_plane<float>(dc_p(c), P, T);
    sdd_dot3p<K>(c, P, Q, ns, r.d);
    SDFK_KLOOP r.d[k] -= SDFK_DQ(k, 3);
    return r;
}
SDFK_DUAL_V_C(dual_prim_uplane) {
    DS<K> r;
    r.v = prim_uplane<float>(dc_p(c), P, T);
    float dd[K];
    sdd_dot3p<K>(c, P, Q, ns, dd);
    sdd_abs<K>(sd_dot3(c.x, c.y, c.z, P[0], P[1], P[2]), dd, r.d);
    SDFK_KLOOP r.d[k] -= SDFK_DQ(k, 3);
    return r;
}
// sqrt(sd_seg3_sq / sd_seg2_sq): S = a(D), ba(D), inv ; D = 3 or 2
template <int K, int D> SDFK_DEV void sdd_segment(const DC<K>& c, const float* __restrict__ S, const float* __restrict__ Q, int ns, float* out) {
#define SDFK_SEG_DP(i, k) ((i) == 0 ? c.dx[k] : ((i) == 1 ? c.dy[k] : c.dz[k]))
    const float p[3] = {c.x, c.y, c.z};
    float pa[3], dot;
#pragma unroll
    for (int i = 0; i < D; ++i) pa[i] = p[i] - S[i];
    if (D == 3) dot = sd_dot3(pa[0], pa[1], pa[2], S[3], S[4], S[5]);
    else dot = sd_dot2(pa[0], pa[1], S[2], S[3]);
    const float t = dot * S[2 * D];
    const float h = sd_clip01(t);
    float dv[3], sq;
#pragma unroll
    for (int i = 0; i < D; ++i) dv[i] = sd_fma(-S[D + i], h, pa[i]);
    if (D == 3) sq = sd_fma(dv[0], dv[0], sd_fma(dv[1], dv[1], dv[2] * dv[2]));
    else sq = sd_fma(dv[0], dv[0], dv[1] * dv[1]);
    const float inv = sdd_rcp(sd_sqrt(sq));
    float dt[K], dh[K];
    SDFK_KLOOP {
        float ddot = 0.0f;
#pragma unroll
        for (int i = 0; i < D; ++i) ddot += (SDFK_SEG_DP(i, k) - SDFK_DQ(k, i)) * S[D + i] + pa[i] * SDFK_DQ(k, D + i);
        dt[k] = ddot * S[2 * D] + dot * SDFK_DQ(k, 2 * D);
    }
    sdd_clip01<K>(t, dt, dh);
    SDFK_KLOOP {
        float acc = 0.0f;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const float dd = (SDFK_SEG_DP(i, k) - SDFK_DQ(k, i)) - SDFK_DQ(k, D + i) * h - S[D + i] * dh[k];
            acc += dv[i] * dd;
        }
        out[k] = acc * inv;
    }
#undef SDFK_SEG_DP
}
SDFK_DUAL_V_C(dual_prim_segment3) {
    DS<K> r;
    r.v = prim_segment3(dc_p(c), P, T);
    sdd_segment<K, 3>(c, P, Q, ns, r.d);
    return r;
}
SDFK_DUAL_V_C(dual_prim_segment2) {
    DS<K> r;
    r.v = prim_segment2(dc_p(c), P, T);
    sdd_segment<K, 2>(c, P, Q, ns, r.d);
    return r;
}
SDFK_DUAL_V_C(dual_prim_cone) {
    DS<K> r;
    r.v = prim_cone<float>(dc_p(c), P, T);
    const float q0 = P[0], q1 = P[1];
    const float w0 = sd_len2(c.x, c.y), w1 = c.z - P[2];
    const float dot = sd_dot2(w0, w1, q0, q1);
    const float u1 = dot * P[3];
    const float t1 = sd_clip01(u1);
    const float ax = sd_fma(-q0, t1, w0), ay = sd_fma(-q1, t1, w1);
    const float u2 = w0 * P[4];
    const float t2 = sd_clip01(u2);
    const float bx = sd_fma(-q0, t2, w0), by = w1 - q1;
    const float da2 = sd_fma(ax, ax, ay * ay), db2 = sd_fma(bx, bx, by * by);
    // Which of the side (a) and the base (b) the tangent follows is decided by the clips where they decide it, not by
    // the two squared distances, which tie in fp32 beside the rim's two normals (see dual_prim_triangle2): both contain
    // the rim, so one that is clipped to the rim is never the nearer of the two.
    const bool ta = (u2 >= 1.0f) ? true : ((u1 >= 1.0f) ? false : da2 <= db2);
    const float s = sd_max(-sd_fma(w0, q1, -w1 * q0), -(w1 - q1));
    const float sg = sd_sign(s);
    const float half_inv = 0.5f * sdd_rcp(sd_sqrt(ta ? da2 : db2));
    float dw0[K], dw1[K], du1[K], du2[K], dt1[K], dt2[K], dA[K], dB[K], dd[K];
    sdd_len2<K>(c.x, c.y, c.dx, c.dy, w0, dw0);
    SDFK_KLOOP {
        dw1[k] = c.dz[k] - SDFK_DQ(k, 2);
        const float ddot = dw0[k] * q0 + w0 * SDFK_DQ(k, 0) + dw1[k] * q1 + w1 * SDFK_DQ(k, 1);
        du1[k] = ddot * P[3] + dot * SDFK_DQ(k, 3);
        du2[k] = dw0[k] * P[4] + w0 * SDFK_DQ(k, 4);
    }
    sdd_clip01<K>(u1, du1, dt1);
    sdd_clip01<K>(u2, du2, dt2);
    SDFK_KLOOP {
        const float dax = dw0[k] - SDFK_DQ(k, 0) * t1 - q0 * dt1[k], day = dw1[k] - SDFK_DQ(k, 1) * t1 - q1 * dt1[k];
        const float dbx = dw0[k] - SDFK_DQ(k, 0) * t2 - q0 * dt2[k], dby = dw1[k] - SDFK_DQ(k, 1);
        dA[k] = 2.0f * (ax * dax + ay * day);
        dB[k] = 2.0f * (bx * dbx + by * dby);
    }
    SDFK_KLOOP dd[k] = ta ? dA[k] : dB[k];
    SDFK_KLOOP r.d[k] = sg * dd[k] * half_inv;
    // Free foot on the side, and the side decides the sign: the value is -cr / |q|, cr = w x q, smooth through the surface.
    // Its tangent is taken from that form: the residual (ax, ay) above is a difference of nearly equal numbers within
    // 1e-7 |w| of the surface, where its direction is rounding noise and its length 0 exactly on it — and a projection
    // onto the surface (sdfk_project.inc) ends there. Both forms are equal in exact arithmetic, parameter terms included.
    const float cr = sd_fma(w0, q1, -w1 * q0);
    if (ta && u1 > 0.0f && u1 < 1.0f && -cr >= -(w1 - q1)) {
        const float rs = sd_sqrt(P[3]), half_inv_rs = 0.5f * sdd_rcp(rs);
        SDFK_KLOOP {
            const float dcr = dw0[k] * q1 + w0 * SDFK_DQ(k, 1) - dw1[k] * q0 - w1 * SDFK_DQ(k, 0);
            r.d[k] = -(dcr * rs + cr * (SDFK_DQ(k, 3) * half_inv_rs));
        }
    }
    // Free foot on the base, and the base decides the sign: bx is 0 but for its rounding, the value is -(w1 - q1).
    if (!ta && u2 > 0.0f && u2 < 1.0f && -(w1 - q1) >= -cr) SDFK_KLOOP r.d[k] = -(dw1[k] - SDFK_DQ(k, 1));
    return r;
}
SDFK_DUAL_V_C(dual_prim_zslab) {
    DS<K> r;
    r.v = prim_zslab<float>(dc_p(c), P, T);
    sdd_abs<K>(c.z, c.dz, r.d);
    SDFK_KLOOP r.d[k] -= SDFK_DQ(k, 0);
    return r;
}
SDFK_DUAL_V_C(dual_prim_box2) {
    DS<K> r;
    r.v = prim_box2<float>(dc_p(c), P, T);
    const float dx = sd_abs(c.x) - P[0], dy = sd_abs(c.y) - P[1];
    const float ax = sd_max0(dx), ay = sd_max0(dy);
    float ddx[K], ddy[K], dax[K], day[K], t1[K], m[K], t2[K];
    sdd_abs<K>(c.x, c.dx, ddx);
    sdd_abs<K>(c.y, c.dy, ddy);
    SDFK_KLOOP ddx[k] -= SDFK_DQ(k, 0), ddy[k] -= SDFK_DQ(k, 1);
    sdd_max0<K>(dx, ddx, dax);
    sdd_max0<K>(dy, ddy, day);
    sdd_len2<K>(ax, ay, dax, day, sd_len2(ax, ay), t1);
    sdd_max<K>(dx, dy, ddx, ddy, m);
    sdd_min0<K>(sd_max(dx, dy), m, t2);
    SDFK_KLOOP r.d[k] = t1[k] + t2[k];
    return r;
}
SDFK_DUAL_V_C(dual_prim_rbox2) {
    DS<K> r;
    r.v = prim_rbox2(dc_p(c), P, T);
    int j = 2;
    j = (c.x > 0.0f) ? 3 : j;
    j = (c.y > 0.0f) ? 4 : j;
    j = (c.x < 0.0f && c.y > 0.0f) ? 5 : j;
    const float rr = P[j];
    const float dx = (sd_abs(c.x) - P[0]) + rr, dy = (sd_abs(c.y) - P[1]) + rr;
    const float ax = sd_max(dx, 0.0f), ay = sd_max(dy, 0.0f);
    float ddx[K], ddy[K], dax[K], day[K], o[K], m[K], u[K];
    sdd_abs<K>(c.x, c.dx, ddx);
    sdd_abs<K>(c.y, c.dy, ddy);
    SDFK_KLOOP {
        const float dr = Q[k * ns + j];
        ddx[k] += dr - SDFK_DQ(k, 0);
        ddy[k] += dr - SDFK_DQ(k, 1);
    }
    sdd_max0<K>(dx, ddx, dax);
    sdd_max0<K>(dy, ddy, day);
    sdd_len2<K>(ax, ay, dax, day, sd_len2(ax, ay), o);
    sdd_max<K>(dx, dy, ddx, ddy, m);
    sdd_min0<K>(sd_max(dx, dy), m, u);
    SDFK_KLOOP r.d[k] = o[k] + u[k] - Q[k * ns + j];
    return r;
}
SDFK_DUAL_V_C(dual_prim_triangle2) {
    DS<K> r;
    r.v = prim_triangle2(dc_p(c), P, T);
    // The tangent follows the nearest edge among those that the clips leave standing, and is the derivative of that
    // edge's own distance. Squared distances alone do not decide it: beside the normal erected at a vertex, the edge with
    // a free foot and its neighbour clipped to that vertex differ by the square of the angle to the normal, which fp32
    // does not resolve (and the offset v - e of an edge clipped to its end cancels), while their gradients differ by the
    // angle itself. Consecutive edges share a vertex, so an edge clipped to its end (t >= 1) is never nearer than the
    // next edge, and one clipped to its start (t <= 0) never nearer than the previous edge unless that one is clipped to
    // its end: such edges are left out. What stands is a free foot, or the offset c - p_i from the vertex itself.
    float tt[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
        tt[i] = sd_dot2(c.x - P[2 * i], c.y - P[2 * i + 1], P[6 + 2 * i], P[7 + 2 * i]) * P[12 + i];
    float dsel = 3.0e38f, kmin = 3.0e38f, cmin = 3.0e38f;
    float ddmin[K];
    SDFK_KLOOP ddmin[k] = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float vx = c.x - P[2 * i], vy = c.y - P[2 * i + 1];
        const float ex = P[6 + 2 * i], ey = P[7 + 2 * i];
        const float dot = sd_dot2(vx, vy, ex, ey);
        const float t = dot * P[12 + i];
        const float h = sd_clip01(t);
        const float qx = sd_fma(-ex, h, vx), qy = sd_fma(-ey, h, vy);
        const float dd = sd_fma(qx, qx, qy * qy);
        float dt[K], dh[K];
        SDFK_KLOOP {
            const float dvx = c.dx[k] - SDFK_DQ(k, 2 * i), dvy = c.dy[k] - SDFK_DQ(k, 2 * i + 1);
            const float ddot = dvx * ex + vx * SDFK_DQ(k, 6 + 2 * i) + dvy * ey + vy * SDFK_DQ(k, 7 + 2 * i);
            dt[k] = ddot * P[12 + i] + dot * SDFK_DQ(k, 12 + i);
        }
        sdd_clip01<K>(t, dt, dh);
        const bool out = t >= 1.0f || (t <= 0.0f && tt[(i + 2) % 3] < 1.0f);
        const float key = out ? 3.0e38f : dd;
        const bool keep = kmin <= key;
        SDFK_KLOOP {
            const float dvx = c.dx[k] - SDFK_DQ(k, 2 * i), dvy = c.dy[k] - SDFK_DQ(k, 2 * i + 1);
            const float dqx = dvx - SDFK_DQ(k, 6 + 2 * i) * h - ex * dh[k], dqy = dvy - SDFK_DQ(k, 7 + 2 * i) * h - ey * dh[k];
            const float ddd = 2.0f * (qx * dqx + qy * dqy);
            ddmin[k] = keep ? ddmin[k] : ddd;
        }
        dsel = keep ? dsel : dd;
        kmin = sd_min(kmin, key);
        cmin = sd_min(cmin, P[15] * sd_fma(vx, ey, -vy * ex));
    }
    const float f = -sd_sign(cmin) * 0.5f * sdd_rcp(sd_sqrt(dsel));
    SDFK_KLOOP r.d[k] = f * ddmin[k];
    return r;
}
SDFK_DUAL_V_C(dual_prim_ngon) {
    DS<K> r;
    r.v = prim_ngon(dc_p(c), P, T);
    float qx, qy, dqx[K], dqy[K];
    if (P[10] > 0.0f) {
        float x = c.x, y = sd_abs(c.y);
        float dx[K], dy[K];
        SDFK_KLOOP dx[k] = c.dx[k];
        sdd_abs<K>(c.y, c.dy, dy);
        const int nf = (int)P[10];
        for (int j = 0; j < nf; ++j) {
            const float yr = sd_fma(P[8], y, -P[9] * x), xr = sd_fma(P[8], x, P[9] * y);
            const bool over = yr >= 0.0f;
            SDFK_KLOOP {
                const float dca = SDFK_DQ(k, 8), dsa = SDFK_DQ(k, 9);
                const float dyr = dca * y + P[8] * dy[k] - dsa * x - P[9] * dx[k];
                const float dxr = dca * x + P[8] * dx[k] + dsa * y + P[9] * dy[k];
                dx[k] = over ? dxr : dx[k];
                dy[k] = over ? dyr : dy[k];
            }
            x = over ? xr : x;
            y = over ? yr : y;
        }
        qx = x - P[0];
        qy = y;
        SDFK_KLOOP dqx[k] = dx[k] - SDFK_DQ(k, 0), dqy[k] = dy[k];
    } else {
        float phi = sd_atan2(c.y, c.x);
        phi = (phi < 0.0f) ? SDFK_TWO_PI + phi : phi;
        const float m = sd_mod(phi, P[1], P[2]);
        const float rr = sd_len2(c.x, c.y);
        float s, co;
        sd_sincos(m, &s, &co);
        qx = co * rr - P[0];
        qy = s * rr;
        float dphi[K], dA[K], dm[K], dr[K];
        sdd_atan2<K>(c.y, c.x, c.dy, c.dx, dphi);
        SDFK_KLOOP dA[k] = SDFK_DQ(k, 1);
        sdd_mod<K>(phi, P[1], P[2], m, dphi, dA, dm);
        sdd_len2<K>(c.x, c.y, c.dx, c.dy, rr, dr);
        SDFK_KLOOP {
            dqx[k] = -s * dm[k] * rr + co * dr[k] - SDFK_DQ(k, 0);
            dqy[k] = co * dm[k] * rr + s * dr[k];
        }
    }
    const float dot = sd_dot2(qx, qy, P[3], P[4]);
    const float h = sd_clip(dot, 0.0f, P[7]);
    const float lx = sd_fma(-P[3], h, qx), ly = sd_fma(-P[4], h, qy);
    const float sg = sd_sign(sd_dot2(qx, qy, P[5], P[6]));
    float ddot[K], zero[K], dl[K], dh[K], dlx[K], dly[K], dlen[K];
    SDFK_KLOOP {
        ddot[k] = dqx[k] * P[3] + qx * SDFK_DQ(k, 3) + dqy[k] * P[4] + qy * SDFK_DQ(k, 4);
        zero[k] = 0.0f;
        dl[k] = SDFK_DQ(k, 7);
    }
    sdd_clip<K>(dot, 0.0f, P[7], ddot, zero, dl, dh);
    SDFK_KLOOP {
        dlx[k] = dqx[k] - SDFK_DQ(k, 3) * h - P[3] * dh[k];
        dly[k] = dqy[k] - SDFK_DQ(k, 4) * h - P[4] * dh[k];
    }
    sdd_len2<K>(lx, ly, dlx, dly, sd_len2(lx, ly), dlen);
    SDFK_KLOOP r.d[k] = dlen[k] * sg;
    return r;
}

// =============================================================================================
// value -> value   DS f(DS a, P, Q, ns)
// =============================================================================================
#define SDFK_DUAL_V_V(name) template <int K> SDFK_DEV DS<K> name(const DS<K>& a, const float* __restrict__ P, \
                                                                  const float* __restrict__ Q, int ns)

SDFK_DUAL_V_V(dual_val_scale) {
    DS<K> r;
    r.v = val_scale<float>(a.v, P);
    SDFK_KLOOP r.d[k] = P[0] * a.d[k] + SDFK_DQ(k, 0) * a.v;
    return r;
}
SDFK_DUAL_V_V(dual_val_subc) {
    DS<K> r;
    r.v = val_subc<float>(a.v, P);
    SDFK_KLOOP r.d[k] = a.d[k] - SDFK_DQ(k, 0);
    return r;
}
SDFK_DUAL_V_V(dual_val_affine) {
    DS<K> r;
    r.v = val_affine<float>(a.v, P);
    SDFK_KLOOP r.d[k] = P[0] * a.d[k] + SDFK_DQ(k, 0) * a.v - SDFK_DQ(k, 1);
    return r;
}
SDFK_DUAL_V_V(dual_val_abs) {
    DS<K> r;
    r.v = val_abs<float>(a.v, P);
    sdd_abs<K>(a.v, a.d, r.d);
    return r;
}
SDFK_DUAL_V_V(dual_val_neg) {
    DS<K> r;
    r.v = val_neg<float>(a.v, P);
    SDFK_KLOOP r.d[k] = -a.d[k];
    return r;
}
SDFK_DUAL_V_V(dual_val_sign) {        // piecewise constant
    DS<K> r;
    r.v = val_sign<float>(a.v, P);
    SDFK_KLOOP r.d[k] = 0.0f;
    return r;
}
SDFK_DUAL_V_V(dual_val_hardbin) {
    DS<K> r;
    r.v = val_hardbin(a.v, P);
    SDFK_KLOOP r.d[k] = 0.0f;
    return r;
}
SDFK_DUAL_V_V(dual_val_expflag) {
    DS<K> r;
    r.v = val_expflag(a.v, P);
    SDFK_KLOOP r.d[k] = 0.0f;
    return r;
}
SDFK_DUAL_V_V(dual_val_onion) {
    DS<K> r;
    r.v = val_onion<float>(a.v, P);
    sdd_abs<K>(a.v, a.d, r.d);
    SDFK_KLOOP r.d[k] -= SDFK_DQ(k, 0);
    return r;
}
SDFK_DUAL_V_V(dual_val_concentric) {
    DS<K> r;
    r.v = val_concentric<float>(a.v, P);
    float d[K];
    SDFK_KLOOP d[k] = a.d[k] - SDFK_DQ(k, 0);
    sdd_abs<K>(a.v - P[0], d, r.d);
    return r;
}
SDFK_DUAL_V_V(dual_val_sigmoid) {     // A g, g = 1 / (1 + e), e = exp((v - shift) k): g' = -g (1 - g) u'
    DS<K> r;
    r.v = val_sigmoid(a.v, P);
    const float e = expf((a.v - P[2]) * P[1]);
    const float g = 1.0f / (1.0f + e);
    const float gg = g * (1.0f - g);
    SDFK_KLOOP {
        const float du = (a.d[k] - SDFK_DQ(k, 2)) * P[1] + (a.v - P[2]) * SDFK_DQ(k, 1);
        r.d[k] = SDFK_DQ(k, 0) * g - P[0] * gg * du;
    }
    return r;
}
SDFK_DUAL_V_V(dual_val_capexp) {
    DS<K> r;
    r.v = val_capexp(a.v, P);
    const float e = expf(a.v * P[1]);
    const float m = sd_min(e, 1.0f);
    const bool te = e <= 1.0f;
    SDFK_KLOOP {
        const float dm = te ? e * (a.d[k] * P[1] + a.v * SDFK_DQ(k, 1)) : 0.0f;
        r.d[k] = SDFK_DQ(k, 0) * m + P[0] * dm;
    }
    return r;
}
SDFK_DUAL_V_V(dual_val_linfall) {
    DS<K> r;
    r.v = val_linfall<float>(a.v, P);
    const float t = 1.0f - a.v * P[1];
    const float cl = sd_clip01(t);
    float dt[K], dcl[K];
    SDFK_KLOOP dt[k] = -(a.d[k] * P[1] + a.v * SDFK_DQ(k, 1));
    sdd_clip01<K>(t, dt, dcl);
    SDFK_KLOOP r.d[k] = dcl[k] * P[0] + cl * SDFK_DQ(k, 0);
    return r;
}
SDFK_DUAL_V_V(dual_val_relu) {
    DS<K> r;
    r.v = val_relu<float>(a.v, P);
    const float u = a.v * P[0];
    float du[K];
    SDFK_KLOOP du[k] = a.d[k] * P[0] + a.v * SDFK_DQ(k, 0);
    sdd_max0<K>(u, du, r.d);
    return r;
}
SDFK_DUAL_V_V(dual_val_smoothrelu) {
    DS<K> r;
    r.v = val_smoothrelu<float>(a.v, P);
    const float u = a.v * P[0];
    const float inv = sdd_rcp(sd_sqrt(sd_fma(u, u, P[1])));
    SDFK_KLOOP {
        const float du = a.d[k] * P[0] + a.v * SDFK_DQ(k, 0);
        const float dq = (u * du + 0.5f * SDFK_DQ(k, 1)) * inv;
        r.d[k] = (du + dq) * 0.5f;
    }
    return r;
}
SDFK_DUAL_V_V(dual_val_slowstart) {
    DS<K> r;
    r.v = val_slowstart<float>(a.v, P);
    const float w = a.v * P[0];
    const float u = sd_max0(w);
    const float inv = sdd_rcp(sd_sqrt(sd_fma(u, u, P[1])));
    float dw[K], du[K];
    SDFK_KLOOP dw[k] = a.d[k] * P[0] + a.v * SDFK_DQ(k, 0);
    sdd_max0<K>(w, dw, du);
    SDFK_KLOOP r.d[k] = (u * du[k] + 0.5f * SDFK_DQ(k, 1)) * inv - SDFK_DQ(k, 2);
    return r;
}
SDFK_DUAL_V_V(dual_val_gauss) {
    DS<K> r;
    r.v = val_gauss(a.v, P);
    const bool clamp = P[2] != 0.0f;
    const float u0 = clamp ? sd_max(a.v, 0.0f) : a.v;
    const float u = u0 * P[1];
    const float e = expf(-4.0f * (u * u));
    float du0[K];
    if (clamp) {
        sdd_max0<K>(a.v, a.d, du0);
    } else {
        SDFK_KLOOP du0[k] = a.d[k];
    }
    SDFK_KLOOP {
        const float du = du0[k] * P[1] + u0 * SDFK_DQ(k, 1);
        r.d[k] = SDFK_DQ(k, 0) * e + P[0] * e * (-8.0f * u * du);
    }
    return r;
}

// =============================================================================================
// (value, value) -> value   DS f(DS a, DS b, P, Q, ns)
// =============================================================================================
#define SDFK_DUAL_V_VV(name) template <int K> SDFK_DEV DS<K> name(const DS<K>& a, const DS<K>& b, const float* __restrict__ P, \
                                                                   const float* __restrict__ Q, int ns)

SDFK_DUAL_V_VV(dual_cmb_mul) {
    DS<K> r;
    r.v = cmb_mul<float>(a.v, b.v, P);
    SDFK_KLOOP r.d[k] = a.d[k] * b.v + a.v * b.d[k];
    return r;
}
SDFK_DUAL_V_VV(dual_cmb_add) {
    DS<K> r;
    r.v = cmb_add<float>(a.v, b.v, P);
    SDFK_KLOOP r.d[k] = a.d[k] + b.d[k];
    return r;
}
SDFK_DUAL_V_VV(dual_cmb_diff) {
    DS<K> r;
    r.v = cmb_diff<float>(a.v, b.v, P);
    SDFK_KLOOP r.d[k] = a.d[k] - b.d[k];
    return r;
}
SDFK_DUAL_V_VV(dual_cmb_min) {
    DS<K> r;
    r.v = cmb_min<float>(a.v, b.v, P);
    sdd_min<K>(a.v, b.v, a.d, b.d, r.d);
    return r;
}
SDFK_DUAL_V_VV(dual_cmb_max) {
    DS<K> r;
    r.v = cmb_max<float>(a.v, b.v, P);
    sdd_max<K>(a.v, b.v, a.d, b.d, r.d);
    return r;
}
SDFK_DUAL_V_VV(dual_cmb_subtract) {
    DS<K> r;
    r.v = cmb_subtract<float>(a.v, b.v, P);
    float nb[K];
    SDFK_KLOOP nb[k] = -b.d[k];
    sdd_max<K>(a.v, -b.v, a.d, nb, r.d);
    return r;
}
// tangent of sd_fma(-(t^E), P[1], min(a, b)), t = max0(P[0] - |a - b|)  (E = 2: smoothmin_poly2, 3: smoothmin_poly3)
template <int K, int E>
SDFK_DEV void sdd_smin(float a, float b, const float* da, const float* db, const float* __restrict__ P,
                       const float* __restrict__ Q, int ns, float* out) {
    const float diff = a - b;
    const float w = P[0] - sd_abs(diff);
    const float t = sd_max0(w);
    float dd[K], dab[K], dw[K], dt[K], dm[K];
    SDFK_KLOOP dd[k] = da[k] - db[k];
    sdd_abs<K>(diff, dd, dab);
    SDFK_KLOOP dw[k] = SDFK_DQ(k, 0) - dab[k];
    sdd_max0<K>(w, dw, dt);
    sdd_min<K>(a, b, da, db, dm);
    const float tp = (E == 2) ? t : t * t;          // t^(E-1)
    const float te = tp * t;                        // t^E
    SDFK_KLOOP out[k] = dm[k] - ((float)E * tp * dt[k] * P[1] + te * SDFK_DQ(k, 1));
}
SDFK_DUAL_V_VV(dual_cmb_smin2) {
    DS<K> r;
    r.v = cmb_smin2<float>(a.v, b.v, P);
    sdd_smin<K, 2>(a.v, b.v, a.d, b.d, P, Q, ns, r.d);
    return r;
}
SDFK_DUAL_V_VV(dual_cmb_smin3) {
    DS<K> r;
    r.v = cmb_smin3<float>(a.v, b.v, P);
    sdd_smin<K, 3>(a.v, b.v, a.d, b.d, P, Q, ns, r.d);
    return r;
}
SDFK_DUAL_V_VV(dual_cmb_smax3) {      // -smin3(-a, -b)
    DS<K> r;
    r.v = cmb_smax3<float>(a.v, b.v, P);
    float na[K], nb[K];
    SDFK_KLOOP na[k] = -a.d[k], nb[k] = -b.d[k];
    sdd_smin<K, 3>(-a.v, -b.v, na, nb, P, Q, ns, r.d);
    SDFK_KLOOP r.d[k] = -r.d[k];
    return r;
}
SDFK_DUAL_V_VV(dual_cmb_ssub3) {      // -smin3(-a, b)
    DS<K> r;
    r.v = cmb_ssub3<float>(a.v, b.v, P);
    float na[K];
    SDFK_KLOOP na[k] = -a.d[k];
    sdd_smin<K, 3>(-a.v, b.v, na, b.d, P, Q, ns, r.d);
    SDFK_KLOOP r.d[k] = -r.d[k];
    return r;
}
// f = (a ea + b eb) / (ea + eb), e_i = exp(x_i - m), x_i = v_i / w: f' = sum w_i (v_i' + (v_i - f) x_i'), w_i = e_i / (ea + eb)
template <int K>
SDFK_DEV void sdd_boltz(float a, float b, const float* da, const float* db, float f, const float* __restrict__ P,
                        const float* __restrict__ Q, int ns, float* out) {
    const float xa = a * P[0], xb = b * P[0];
    const float m = sd_max(xa, xb);
    const float ea = expf(xa - m), eb = expf(xb - m);
    const float inv = 1.0f / (ea + eb);
    const float wa = ea * inv, wb = eb * inv;
    SDFK_KLOOP {
        const float dxa = da[k] * P[0] + a * SDFK_DQ(k, 0), dxb = db[k] * P[0] + b * SDFK_DQ(k, 0);
        out[k] = wa * (da[k] + (a - f) * dxa) + wb * (db[k] + (b - f) * dxb);
    }
}
SDFK_DUAL_V_VV(dual_cmb_boltz) {
    DS<K> r;
    r.v = cmb_boltz(a.v, b.v, P);
    sdd_boltz<K>(a.v, b.v, a.d, b.d, r.v, P, Q, ns, r.d);
    return r;
}
SDFK_DUAL_V_VV(dual_cmb_boltzsub) {
    DS<K> r;
    r.v = cmb_boltzsub(a.v, b.v, P);
    float nb[K];
    SDFK_KLOOP nb[k] = -b.d[k];
    sdd_boltz<K>(a.v, -b.v, a.d, nb, r.v, P, Q, ns, r.d);
    return r;
}
SDFK_DUAL_V_VV(dual_cmb_extrude) {
    DS<K> r;
    r.v = cmb_extrude<float>(a.v, b.v, P);
    const float m = sd_max(a.v, b.v);
    const float pa = sd_max0(a.v), pb = sd_max0(b.v);
    float dm[K], t1[K], dpa[K], dpb[K], t2[K];
    sdd_max<K>(a.v, b.v, a.d, b.d, dm);
    sdd_min0<K>(m, dm, t1);
    sdd_max0<K>(a.v, a.d, dpa);
    sdd_max0<K>(b.v, b.d, dpb);
    sdd_len2<K>(pa, pb, dpa, dpb, sd_len2(pa, pb), t2);
    SDFK_KLOOP r.d[k] = t1[k] + t2[k];
    return r;
}

// =============================================================================================
// THE table: which opcodes have a dual rule (and which function). The kernel's switch, the library's refusal
// (sdfk_program_jvp_check / sdfk_dual_has_rule) and DESIGN.md's list all come from here. Opcodes absent from it —
// P_BRAID P_INFCONE P_SOLIDANGLE P_TRIANGLE3 P_QUAD3 P_SECTOR P_INFSECTOR P_NEUCIRCLE, the table-driven ones and
// V_FIELD — are refused.
// =============================================================================================
#define SDFK_DUAL_TABLE(X)                                                                                      \
    X(MOVC, C_C, dual_op_movc) X(XFORM, C_C, dual_op_xform) X(XLATE, C_C, dual_op_xlate) X(LIN3, C_C, dual_op_lin3)   \
    X(CSCALE, C_C, dual_op_cscale) X(ELONGATE, C_C, dual_op_elongate) X(REVOLVE, C_C, dual_op_revolve)               \
    X(ROT2D, C_C, dual_op_rot2d) X(AXREV, C_C, dual_op_axrev) X(ZEROZ, C_C, dual_op_zeroz)                           \
    X(TWIST, C_C, dual_op_twist) X(BEND, C_C, dual_op_bend) X(INFREP, C_C, dual_op_infrep)                           \
    X(FINREP, C_C, dual_op_finrep) X(SYMMETRY, C_C, dual_op_symmetry) X(FOLDX, C_C, dual_op_foldx)                   \
    X(ROTSYM, C_C, dual_op_rotsym) X(LININST, C_C, dual_op_lininst)                                                  \
    X(P_AXIS, V_C, dual_prim_axis) X(P_SPHERE, V_C, dual_prim_sphere) X(P_CYLINDER, V_C, dual_prim_cylinder)         \
    X(P_BOX, V_C, dual_prim_box) X(P_TORUS, V_C, dual_prim_torus) X(P_CHAINLINK, V_C, dual_prim_chainlink)           \
    X(P_ARC3D, V_C, dual_prim_arc3d) X(P_PLANE, V_C, dual_prim_plane) X(P_UPLANE, V_C, dual_prim_uplane)             \
    X(P_SEGMENT3, V_C, dual_prim_segment3) X(P_CONE, V_C, dual_prim_cone) X(P_ZSLAB, V_C, dual_prim_zslab)           \
    X(P_CIRCLE, V_C, dual_prim_circle) X(P_BOX2, V_C, dual_prim_box2) X(P_SEGMENT2, V_C, dual_prim_segment2)         \
    X(P_RBOX2, V_C, dual_prim_rbox2) X(P_TRIANGLE2, V_C, dual_prim_triangle2) X(P_ARC2, V_C, dual_prim_arc2)         \
    X(P_NGON, V_C, dual_prim_ngon)                                                                                  \
    X(VSCALE, V_V, dual_val_scale) X(VSUBC, V_V, dual_val_subc) X(VAFFINE, V_V, dual_val_affine)                     \
    X(VABS, V_V, dual_val_abs) X(VNEG, V_V, dual_val_neg) X(VSIGN, V_V, dual_val_sign) X(VONION, V_V, dual_val_onion) \
    X(VCONCENTRIC, V_V, dual_val_concentric) X(VSIGMOID, V_V, dual_val_sigmoid) X(VCAPEXP, V_V, dual_val_capexp)     \
    X(VHARDBIN, V_V, dual_val_hardbin) X(VLINFALL, V_V, dual_val_linfall) X(VRELU, V_V, dual_val_relu)               \
    X(VSMOOTHRELU, V_V, dual_val_smoothrelu) X(VSLOWSTART, V_V, dual_val_slowstart) X(VGAUSS, V_V, dual_val_gauss)   \
    X(VEXPFLAG, V_V, dual_val_expflag)                                                                              \
    X(VMUL, V_VV, dual_cmb_mul) X(VADD, V_VV, dual_cmb_add) X(VDIFF, V_VV, dual_cmb_diff) X(VMIN, V_VV, dual_cmb_min) \
    X(VMAX, V_VV, dual_cmb_max) X(VSUBTRACT, V_VV, dual_cmb_subtract) X(SMIN2, V_VV, dual_cmb_smin2)                 \
    X(SMIN3, V_VV, dual_cmb_smin3) X(SMAX3, V_VV, dual_cmb_smax3) X(SSUB3, V_VV, dual_cmb_ssub3)                     \
    X(BOLTZ, V_VV, dual_cmb_boltz) X(BOLTZSUB, V_VV, dual_cmb_boltzsub) X(EXTRUDE, V_VV, dual_cmb_extrude)

#endif  // SDFK_DUALDEV_H
