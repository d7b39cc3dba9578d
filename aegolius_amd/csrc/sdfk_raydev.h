// sdfk_raydev.h — sphere tracing of one program: the marching loops, the ray sources and the stencil normals. Shared
// (like sdfk_access.h) by the interpreter march kernel (sdfk_rays.inc) and, as embedded text, by the hiprtc-specialised
// ones (SDFK_FL_RAYS, SDFK_FL_SPANS, SDFK_FL_SECONDARY), so that the marching arithmetic is ONE piece of text: both kernels give the same bits.
// One interface for every march: sdfk_march(src, field, opts, out), overloaded on the output record — SdfkHitOut: the first
// hit (sdfk_trace, the rule below), SdfkSpanOut: every crossing and the chord (sdfk_trace_spans, the rule further down),
// SdfkVisOut: how much of a segment is free of the solid (sdfk_trace_visibility), SdfkAoOut: how open the half-space above
// a surface point is (sdfk_trace_occlusion) — the two secondary marches, at the end of this file.
//
// The marching rule (aegolius_amd/render.py states it for users; tests/render_reference.py is its float64 copy):
//     t = t_min
//     repeat at most max_steps times:
//         f   = field(o + t d)                     fp32: fmaf(t, d, o) per component
//         thr = max(eps, cone t)
//         if f <= thr: hit, stop                   (steps = advances made so far: 0 for a ray that starts on the solid)
//         t   = fmaf(f, 1 / L, t)                  1 / L rounded once on the host; steps += 1
//         if t > t_max: miss, stop
//     otherwise: step limit
// One ray per lane. The loop runs while any lane of the wave still marches: the trip count is wave-uniform, so the
// evaluator's code words stay scalar loads; lanes that have finished evaluate along and are masked out of every update.
//
// The wave-level hook. Before every evaluation the loop calls field.prepare(p, t, active, reach) in wave-uniform control
// flow: `active` marks the lanes whose value will be used (the marching lanes; at the normal, the lanes that hit), and
// the evaluations that follow stay within `reach` of this lane's p (0 along the ray; the stencil's reach at the normal).
// A field may bound the active points of the wave and cull its members for them (the specialised chain-mode kernels:
// sdfk_raycull.h, SdfkCullField); the interpreter's field ignores the call. The hook returns nothing and the value of
// an active lane must not depend on it: the marching arithmetic below is the same with and without.
#ifndef SDFK_RAYDEV_H
#define SDFK_RAYDEV_H

#define SDFK_RAY_BLOCK 256
#define SDFK_RAY_MISS 0u
#define SDFK_RAY_HIT 1u
#define SDFK_RAY_LIMIT 2u

struct sdfk_rayopts {
    float t_min, t_max, eps, cone, inv_lip;
    int max_steps;
};
// Camera record. Pixel (ix, iy), iy = 0 the TOP row, a = (2 ix + 1) / W - 1, b = 1 - (2 iy + 1) / H:
//   perspective : o = eye,                 d = (fwd + a du + b dv) / |fwd + a du + b dv|
//   orthographic: o = eye + a du + b dv,   d = fwd
// fwd is a unit vector, du / dv the right / up unit vectors scaled by half the extent of the image plane (at distance
// 1 for the perspective camera).
struct sdfk_camera {
    float eye[3], fwd[3], du[3], dv[3];
    float inv_w, inv_h;        // 1 / W, 1 / H rounded to fp32 on the host
    int width, height, ortho;
};

struct SdfkRaysArray {      // two (3, n) arrays, rows strided like d_co everywhere else; ray i on lane i of the launch
    const float* __restrict__ o;
    long long ostride;
    const float* __restrict__ d;
    long long dstride;
    long long n;
};
struct SdfkRaysCamera {     // rays generated from the record; every wave owns one tile of 8 x 8 pixels
    sdfk_camera cam;
};

// What a march writes per ray, and with it which march sdfk_march runs.
struct SdfkHitOut {         // first hit: where the ray stopped, 0 miss / 1 hit / 2 step limit, advances made
    float* __restrict__ t;
    unsigned char* __restrict__ status;
    int* __restrict__ steps;
    float* __restrict__ n;  // the stencil normal, three rows nstride apart; null: none
    long long nstride;
};
struct SdfkSpanOut {        // spans: length inside the solid, all crossings counted, status (| SDFK_SPAN_INSIDE0), evaluations
    float* __restrict__ chord;
    int* __restrict__ count;
    unsigned char* __restrict__ status;
    int* __restrict__ steps;
    float* __restrict__ cross;  // the first max_crossings crossings, rows cstride apart (not read when max_crossings is 0)
    long long cstride;
    int max_crossings;
};
struct SdfkVisOut {         // visibility: what the ray saw of the light in [0, 1], 0 clear / 1 blocked / 2 step limit, advances made
    float softness;         // k of the penumbra estimate; 0: hard, vis is 0 or 1
    const float* __restrict__ limits;   // the end of every ray (a point light's distance), t_max where that is smaller; null: t_max
    float* __restrict__ vis;
    unsigned char* __restrict__ status;
    int* __restrict__ steps;
};
#define SDFK_AO_MAX_SAMPLES 16
struct SdfkAoOut {          // ambient occlusion of the points `o` with the unit normals `d` of the source
    float inv_m, inv_radius;    // 1 / samples and 1 / radius rounded to fp32 on the host (radius: opts.t_max, samples: opts.max_steps)
    float strength;
    float* __restrict__ ao;
};

// -> is there a ray on this lane; its origin, direction and the index its results are stored at
static __device__ __forceinline__ bool sdfk_ray_load(const SdfkRaysArray& s, V3& o, V3& d, long long& at) {
    at = (long long)sdfk_bx() * SDFK_RAY_BLOCK + sdfk_tx();
    o = {0.0f, 0.0f, 0.0f};
    d = {0.0f, 0.0f, 0.0f};
    if (at >= s.n) return false;
    o = {s.o[at], s.o[s.ostride + at], s.o[2 * s.ostride + at]};
    d = {s.d[at], s.d[s.dstride + at], s.d[2 * s.dstride + at]};
    return true;
}
static __device__ __forceinline__ bool sdfk_ray_load(const SdfkRaysCamera& s, V3& o, V3& d, long long& at) {
    const sdfk_camera& c = s.cam;
    const unsigned tiles_x = ((unsigned)c.width + 7u) >> 3;
    const unsigned tile = sdfk_bx() * (SDFK_RAY_BLOCK / 64) + (sdfk_tx() >> 6);   // wave-uniform
    const unsigned ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const unsigned lane = sdfk_tx() & 63u;
    const unsigned ix = tx * 8u + (lane & 7u), iy = ty * 8u + (lane >> 3);
    at = (long long)iy * c.width + ix;
    o = {0.0f, 0.0f, 0.0f};
    d = {0.0f, 0.0f, 0.0f};
    if (ix >= (unsigned)c.width || iy >= (unsigned)c.height) return false;
    const float a = fmaf((float)(2u * ix + 1u), c.inv_w, -1.0f);
    const float b = fmaf(-(float)(2u * iy + 1u), c.inv_h, 1.0f);
    const V3 q = {fmaf(b, c.dv[0], a * c.du[0]), fmaf(b, c.dv[1], a * c.du[1]), fmaf(b, c.dv[2], a * c.du[2])};
    if (c.ortho) {
        o = {c.eye[0] + q.x, c.eye[1] + q.y, c.eye[2] + q.z};
        d = {c.fwd[0], c.fwd[1], c.fwd[2]};
    } else {
        const V3 w = {c.fwd[0] + q.x, c.fwd[1] + q.y, c.fwd[2] + q.z};
        const float inv = 1.0f / sqrtf(fmaf(w.z, w.z, fmaf(w.y, w.y, w.x * w.x)));
        o = {c.eye[0], c.eye[1], c.eye[2]};
        d = {w.x * inv, w.y * inv, w.z * inv};
    }
    return true;
}

// Width of the normal stencil at a hit: the hit threshold there, floored at 2^-16 max(|x|, |y|, |z|) — 128 fp32
// spacings of the largest coordinate, so that the four stencil points are distinct numbers and the difference of their
// field values keeps about 7 bits (aegolius_amd.render.stencil_width is the same arithmetic on the host).
static __device__ __forceinline__ float sdfk_ray_stencil_width(float thr, V3 p) {
    const float m = fmaxf(fmaxf(fabsf(p.x), fabsf(p.y)), fabsf(p.z));
    return fmaxf(thr, 1.52587890625e-05f * m);
}

// FIELD: float operator()(V3) const — the program at one point (interpreter switch or the generated sdfk_point<float>);
//        void prepare(V3 p, float t, bool active, float reach) const — the wave-level hook (see the head of this file)
template <typename SRC, typename FIELD>
static __device__ __forceinline__ void sdfk_trace(const SRC& src, const FIELD& field, const sdfk_rayopts R,
                                                  float* __restrict__ out_t, unsigned char* __restrict__ out_status,
                                                  int* __restrict__ out_steps, float* __restrict__ out_n,
                                                  long long nstride) {
    V3 o, d;
    long long at;
    const bool live = sdfk_ray_load(src, o, d, at);
    float t = R.t_min, thr = R.eps;
    unsigned status = SDFK_RAY_LIMIT;
    int steps = 0;
    bool marching = live;
    for (int it = 0; it < R.max_steps; ++it) {
        if (!__any(marching)) break;
        const V3 p = {fmaf(t, d.x, o.x), fmaf(t, d.y, o.y), fmaf(t, d.z, o.z)};
        field.prepare(p, t, marching, 0.0f);
        const float f = field(p);
        if (marching) {
            thr = fmaxf(R.eps, R.cone * t);
            if (f <= thr) {
                status = SDFK_RAY_HIT;
                marching = false;
            } else {
                t = fmaf(f, R.inv_lip, t);
                ++steps;
                if (t > R.t_max) {
                    status = SDFK_RAY_MISS;
                    marching = false;
                }
            }
        }
    }
    if (live) {
        out_t[at] = t;
        out_status[at] = (unsigned char)status;
        out_steps[at] = steps;
    }
    if (!out_n) return;                                       // wave-uniform (a kernel argument)
    // four-point tetrahedron difference at the hit: g = sum_i k_i f(p + h k_i), k = (+--), (--+), (-+-), (+++), summed
    // in that order; g / 4h is the gradient, the normal is g / |g|. Lanes that did not hit store the zero vector.
    const bool hit = live && status == SDFK_RAY_HIT;
    V3 nrm = {0.0f, 0.0f, 0.0f};
    if (__any(hit)) {
        const V3 p = {fmaf(t, d.x, o.x), fmaf(t, d.y, o.y), fmaf(t, d.z, o.z)};
        const float h = sdfk_ray_stencil_width(thr, p);
        // the four stencil points lie within sqrt(3) h of p, plus the rounding of p + h k: at most 2^-24 max|p| <= 2^-8 h
        // per component by the floor of h — 1.75 > sqrt(3) (1 + 2^-8)
        field.prepare(p, t, hit, 1.75f * h);
        V3 g = {0.0f, 0.0f, 0.0f};
        _Pragma("unroll 1") for (int k = 0; k < 4; ++k) {       // (one call site: the body is inlined once, not four times)
            const float kx = (k == 0 || k == 3) ? 1.0f : -1.0f, ky = (k >= 2) ? 1.0f : -1.0f,
                        kz = (k == 1 || k == 3) ? 1.0f : -1.0f;
            const float f = field(V3{fmaf(kx, h, p.x), fmaf(ky, h, p.y), fmaf(kz, h, p.z)});
            g = {g.x + kx * f, g.y + ky * f, g.z + kz * f};
        }
        const float len = sqrtf(fmaf(g.z, g.z, fmaf(g.y, g.y, g.x * g.x)));
        if (hit && len > 0.0f) {
            const float inv = 1.0f / len;
            nrm = {g.x * inv, g.y * inv, g.z * inv};
        }
    }
    if (live) {
        out_n[at] = nrm.x;
        out_n[nstride + at] = nrm.y;
        out_n[2 * nstride + at] = nrm.z;
    }
}

// ---- spans: the march that goes on through the surface ---------------------------------------------------------------------
// Every entry and exit crossing of a ray with the solid { f <= 0 }, and the length of the ray inside it (the chord). The
// rule (aegolius_amd/render.py states it for users; tests/spans_reference.py is its float64 copy), per ray, in fp32:
//     t = t_min; count = 0; chord = 0
//     repeat at most max_steps times (evaluation index e = 0, 1, ...):
//         f      = field(o + t d)                              fmaf(t, d, o) per component, as above
//         inside = (f <= 0)
//         if e == 0: was = inside; inside0 = inside; t_in = t_min          starting inside is not a crossing
//         else if inside != was:                                          a sign change between t_prev and t
//             tc = fmaf(t - t_prev, |f_prev| / (|f_prev| + |f|), t_prev)      secant; the denominator is > 0
//             if count < K: crossings[count] = tc
//             count += 1
//             if inside: t_in = tc   else: chord += tc - t_in
//             was = inside
//         thr    = max(eps, cone t)
//         t_prev = t; f_prev = f
//         t_next = t + max(|f| * (1 / L), thr)                 1 / L rounded once on the host; steps += 1
//         if not (t_next > t): status = LIMIT; stop            no progress in fp32: never loop in place
//         t = t_next
//         if t > t_max: if was: chord += t_max - t_in;  status = COMPLETE; stop
//     otherwise: status = LIMIT
//     on LIMIT, either way: if was: chord += t_prev - t_in     (t_prev: the last evaluated parameter)
// A step of |f| / L cannot cross the surface, so the sign changes only inside floor steps of length thr: the state at every
// evaluated point is the field's own, every crossing is bracketed within thr, and only features thinner than thr along
// the ray can be missed, as a pair. The loop has the wave-uniform shape of sdfk_trace: it runs while any lane marches, calls
// the hook before every evaluation, and finished lanes evaluate along, masked out of every update (e is the trip count,
// the same number on every lane). A crossing is stored when it is found — row k of ray i at k * cstride + i, one
// contiguous line per wave — so that no lane keeps an indexed array; rows from `count` on are not written.
#define SDFK_SPAN_COMPLETE 0u
#define SDFK_SPAN_LIMIT 2u
#define SDFK_SPAN_INSIDE0 4u       // added to the status of a ray that is inside the solid at t_min
#define SDFK_SPAN_MAX_CROSSINGS 32

template <typename SRC, typename FIELD>
static __device__ __forceinline__ void sdfk_trace_spans(const SRC& src, const FIELD& field, const sdfk_rayopts R,
                                                        const int max_crossings, float* __restrict__ out_chord,
                                                        int* __restrict__ out_count, unsigned char* __restrict__ out_status,
                                                        int* __restrict__ out_steps, float* __restrict__ out_cross,
                                                        long long cstride) {
    V3 o, d;
    long long at;
    const bool live = sdfk_ray_load(src, o, d, at);
    float t = R.t_min, t_prev = R.t_min, f_prev = 0.0f, t_in = R.t_min, chord = 0.0f;
    unsigned status = SDFK_SPAN_LIMIT;
    int steps = 0, count = 0;
    bool was = false, inside0 = false;
    bool marching = live;
    for (int it = 0; it < R.max_steps; ++it) {
        if (!__any(marching)) break;
        const V3 p = {fmaf(t, d.x, o.x), fmaf(t, d.y, o.y), fmaf(t, d.z, o.z)};
        field.prepare(p, t, marching, 0.0f);
        const float f = field(p);
        if (marching) {
            const bool inside = f <= 0.0f;
            if (it == 0) {
                was = inside;
                inside0 = inside;
            } else if (inside != was) {
                const float af = fabsf(f_prev);
                const float tc = fmaf(t - t_prev, af / (af + fabsf(f)), t_prev);
                if (count < max_crossings) out_cross[(long long)count * cstride + at] = tc;
                ++count;
                if (inside) t_in = tc;
                else chord += tc - t_in;
                was = inside;
            }
            const float thr = fmaxf(R.eps, R.cone * t);
            t_prev = t;
            f_prev = f;
            const float t_next = t + fmaxf(fabsf(f) * R.inv_lip, thr);
            ++steps;
            if (!(t_next > t)) {
                marching = false;                               // (status stays LIMIT)
            } else {
                t = t_next;
                if (t > R.t_max) {
                    if (was) chord += R.t_max - t_in;
                    status = SDFK_SPAN_COMPLETE;
                    marching = false;
                }
            }
        }
    }
    if (live) {
        if (status == SDFK_SPAN_LIMIT && was) chord += t_prev - t_in;
        out_chord[at] = chord;
        out_count[at] = count;
        out_status[at] = (unsigned char)(status | (inside0 ? SDFK_SPAN_INSIDE0 : 0u));
        out_steps[at] = steps;
    }
}

// ---- secondary marches: what a surface point sees ------------------------------------------------------------------------------
// Visibility of a segment (aegolius_amd/render.py states the rule for users; tests/secondary_reference.py is its float64
// copy), per ray, in fp32:
//     t = t_min; vis = 1; t_end = limits ? min(t_max, limits[i]) : t_max
//     repeat at most max_steps times:
//         f   = field(o + t d)                           fmaf(t, d, o) per component, as above
//         thr = max(eps, cone t)
//         if f <= thr: vis = 0; status = HIT; stop       blocked
//         if k > 0: vis = min(vis, k (f / L) / t)        the penumbra estimate; t = 0 gives +inf, since f > thr >= 0
//         t   = fmaf(f, 1 / L, t); steps += 1
//         if t > t_end: status = MISS; stop              clear
//     otherwise: status = LIMIT                          vis is what was seen so far, never folded into 0 or 1
// The advance, the hit test and the miss test are sdfk_trace's: with limits null, status, steps and the final t are those
// of the first-hit march, whatever k. f / L is the radius of a ball around o + t d that is free of the solid, so
// k (f / L) / t compares the angular size of the free cone around the ray with 1 / k: a ray that passes closer to the solid
// than t / k anywhere sees less than the whole light. t_min >= 0 (the entry point's check) keeps vis in [0, 1] without a
// clamp. The shape is sdfk_trace's: the loop runs while any lane marches, the hook is called before the one evaluation,
// finished lanes evaluate along, masked.
template <typename SRC, typename FIELD>
static __device__ __forceinline__ void sdfk_trace_visibility(const SRC& src, const FIELD& field, const sdfk_rayopts R,
                                                             const float softness, const float* __restrict__ limits,
                                                             float* __restrict__ out_vis, unsigned char* __restrict__ out_status,
                                                             int* __restrict__ out_steps) {
    V3 o, d;
    long long at;
    const bool live = sdfk_ray_load(src, o, d, at);
    float t_end = R.t_max;
    if (limits && live) t_end = fminf(R.t_max, limits[at]);    // (limits: wave-uniform, a kernel argument)
    float t = R.t_min, vis = 1.0f;
    unsigned status = SDFK_RAY_LIMIT;
    int steps = 0;
    bool marching = live;
    for (int it = 0; it < R.max_steps; ++it) {
        if (!__any(marching)) break;
        const V3 p = {fmaf(t, d.x, o.x), fmaf(t, d.y, o.y), fmaf(t, d.z, o.z)};
        field.prepare(p, t, marching, 0.0f);
        const float f = field(p);
        if (marching) {
            const float thr = fmaxf(R.eps, R.cone * t);
            if (f <= thr) {
                vis = 0.0f;
                status = SDFK_RAY_HIT;
                marching = false;
            } else {
                if (softness > 0.0f) vis = fminf(vis, softness * (f * R.inv_lip) / t);
                t = fmaf(f, R.inv_lip, t);
                ++steps;
                if (t > t_end) {
                    status = SDFK_RAY_MISS;
                    marching = false;
                }
            }
        }
    }
    if (live) {
        out_vis[at] = vis;
        out_status[at] = (unsigned char)status;
        out_steps[at] = steps;
    }
}

// Ambient occlusion of a surface point p with the unit normal n (the source's o and d), m = samples, in fp32:
//     occ = 0
//     for i = 1 .. m:
//         h   = radius (float)i (1 / m)                  1 / m rounded once on the host
//         f   = field(p + h n)                           fmaf(h, n, p) per component
//         occ = fmaf(2^-i, max(0, h - f / L), occ)       f * (1 / L), 1 / L rounded once on the host
//     ao = min(1, max(0, 1 - strength occ (1 / radius)))       1 / radius rounded once on the host
// Above a plane f / L = h at every sample and ao = 1; whatever else comes within h of the sample lowers f and darkens the
// point, near samples counting most. Every lane has the same trip count, so the loop needs no ballot: the hook is called
// with the lanes that hold a point, before the one evaluation (a wave without a point does nothing at all).
template <typename SRC, typename FIELD>
static __device__ __forceinline__ void sdfk_trace_occlusion(const SRC& src, const FIELD& field, const sdfk_rayopts R,
                                                            const float inv_m, const float inv_radius, const float strength,
                                                            float* __restrict__ out_ao) {
    V3 p, n;
    long long at;
    const bool live = sdfk_ray_load(src, p, n, at);
    if (!__any(live)) return;
    float occ = 0.0f, w = 1.0f;
    _Pragma("unroll 1") for (int i = 1; i <= R.max_steps; ++i) {    // (one call site of the field)
        const float h = R.t_max * (float)i * inv_m;
        const V3 q = {fmaf(h, n.x, p.x), fmaf(h, n.y, p.y), fmaf(h, n.z, p.z)};
        field.prepare(q, h, live, 0.0f);
        const float f = field(q);
        w *= 0.5f;                                                  // 2^-i, exact
        occ = fmaf(w, fmaxf(0.0f, h - f * R.inv_lip), occ);
    }
    if (live) out_ao[at] = fminf(1.0f, fmaxf(0.0f, 1.0f - strength * occ * inv_radius));
}

// The one interface of the marches: the output record selects the loop.
template <typename SRC, typename FIELD>
static __device__ __forceinline__ void sdfk_march(const SRC& src, const FIELD& field, const sdfk_rayopts R, const SdfkHitOut out) {
    sdfk_trace(src, field, R, out.t, out.status, out.steps, out.n, out.nstride);
}
template <typename SRC, typename FIELD>
static __device__ __forceinline__ void sdfk_march(const SRC& src, const FIELD& field, const sdfk_rayopts R, const SdfkSpanOut out) {
    sdfk_trace_spans(src, field, R, out.max_crossings, out.chord, out.count, out.status, out.steps, out.cross, out.cstride);
}
template <typename SRC, typename FIELD>
static __device__ __forceinline__ void sdfk_march(const SRC& src, const FIELD& field, const sdfk_rayopts R, const SdfkVisOut out) {
    sdfk_trace_visibility(src, field, R, out.softness, out.limits, out.vis, out.status, out.steps);
}
template <typename SRC, typename FIELD>
static __device__ __forceinline__ void sdfk_march(const SRC& src, const FIELD& field, const sdfk_rayopts R, const SdfkAoOut out) {
    sdfk_trace_occlusion(src, field, R, out.inv_m, out.inv_radius, out.strength, out.ao);
}

// One specialised kernel of the generated text: NAME runs the march OUT (SDFK_HIT, SDFK_SPAN, SDFK_VIS or SDFK_AO) on the rays of SRC
// (SDFK_ARRAY: SdfkRaysArray; SDFK_CAMERA: the camera record, wrapped into SdfkRaysCamera) around FIELD (SDFK_FIELD_PLAIN,
// or SDFK_FIELD_CULL of sdfk_raycull.h). Parameters: (PRM, TAB, the source, opts, the march's outputs, STATS) — STATS: the
// counters of the statistics build of the culled first-hit kernels, null in every other launch. The outputs are flat
// parameters handed straight to the loop: a by-value record spilled SGPRs (profiles/ray_family_refactor.txt).
#define SDFK_ARRAY_PARAM SdfkRaysArray src
#define SDFK_ARRAY_SOURCE
#define SDFK_CAMERA_PARAM sdfk_camera cam
#define SDFK_CAMERA_SOURCE const SdfkRaysCamera src = {cam};
#define SDFK_HIT_PARAMS                                                                                           \
    float *__restrict__ out_t, unsigned char *__restrict__ out_status, int *__restrict__ out_steps,               \
        float *__restrict__ out_n, long long nstride
#define SDFK_HIT_MARCH sdfk_trace(src, field, opts, out_t, out_status, out_steps, out_n, nstride)
#define SDFK_SPAN_PARAMS                                                                                          \
    int max_crossings, float *__restrict__ out_chord, int *__restrict__ out_count,                                \
        unsigned char *__restrict__ out_status, int *__restrict__ out_steps, float *__restrict__ out_cross,       \
        long long cstride
#define SDFK_SPAN_MARCH \
    sdfk_trace_spans(src, field, opts, max_crossings, out_chord, out_count, out_status, out_steps, out_cross, cstride)
#define SDFK_VIS_PARAMS                                                                                           \
    float softness, const float *__restrict__ limits, float *__restrict__ out_vis,                                \
        unsigned char *__restrict__ out_status, int *__restrict__ out_steps
#define SDFK_VIS_MARCH sdfk_trace_visibility(src, field, opts, softness, limits, out_vis, out_status, out_steps)
#define SDFK_AO_PARAMS float inv_m, float inv_radius, float strength, float *__restrict__ out_ao
#define SDFK_AO_MARCH sdfk_trace_occlusion(src, field, opts, inv_m, inv_radius, strength, out_ao)
#define SDFK_FIELD_PLAIN const SdfkSpecField field = {PRM, TAB}
#define SDFK_MARCH_KERNEL(NAME, SRC, OUT, FIELD)                                                                   \
    extern "C" __global__ __launch_bounds__(SDFK_RAY_BLOCK) void NAME(const float* __restrict__ PRM,              \
                                                                      const float* __restrict__ TAB, SRC##_PARAM, \
                                                                      sdfk_rayopts opts, OUT##_PARAMS,            \
                                                                      unsigned long long* STATS) {                \
        FIELD;                                                                                                     \
        SRC##_SOURCE                                                                                               \
        OUT##_MARCH;                                                                                               \
    }

#endif  // SDFK_RAYDEV_H
