// sdfk_rays.inc — sphere tracing of a program (included at the end of sdfk.hip; the loop itself: sdfk_raydev.h).
//
//   * sdfk_rays_interp_kernel<NC, NV, SRC> : the interpreter's register machine as a __device__ evaluation of ONE point
//     (SdfkInterpField: the opcode switch instantiated from sdfk_ops.def once more, as the dual and adjoint kernels do),
//     called from the marching loop. One ray per lane; the code words are wave-uniform (scalar loads) because the
//     loop's trip count is. SRC = SdfkRaysArray (two (3, n) arrays) or SdfkRaysCamera (rays generated from the camera
//     record, one 8 x 8 pixel tile per wave). Register files as in sdfk_interp_kernel, and with the same outcome as its
//     one-point-per-lane instantiations (compiler's resource remarks, all four instances: 57 VGPRs, 8 waves per SIMD):
//     the small coordinate file stays in VGPRs and its three value registers, indexed by the wave-uniform operand
//     fields, take 16 bytes of scratch per lane (sdfk_interp_kernel<1, 2, 3>: 16 as well); the full file takes 128.
//   * the specialised flavour (SDFK_FL_RAYS, sdfk_codegen.cpp) wraps the generated sdfk_point<float> in the same loop;
//     long hard unions (chain mode) get a second pair of kernels there that folds the chain over per-wave survivor
//     lists in LDS (kRaysCull) — what SPECIALIZED / AUTO launch, NOCULL the plain pair; same bits.
//   * sdfk_spans_interp_kernel / SDFK_FL_SPANS: the same field objects inside sdfk_trace_spans, the march that goes on
//     through the surface (every crossing, the chord); selected, culled and served by the interpreter exactly as above.
// Outputs per ray: t (fp32), status (1 byte: 0 miss, 1 hit, 2 step limit), steps (int32), optionally the stencil normal
// (three strided rows). Plain vector stores, written once; no atomics, no LDS.
#include "sdfk_raydev.h"

template <int NC, int NV>
struct SdfkInterpField {
    const uint2* __restrict__ code;
    int n_instr;
    const float* __restrict__ prm;
    const float* __restrict__ tab;
    int result_reg;
    __device__ __forceinline__ void prepare(V3, float, bool, float) const {}   // (the wave-level hook: nothing to cull here)
    __device__ __forceinline__ float operator()(V3 p0) const {
        constexpr bool SPLIT = NC <= SDFK_NC_SMALL;             // (see sdfk_interp_kernel)
        float CX[SPLIT ? NC : 1], CY[SPLIT ? NC : 1], CZ[SPLIT ? NC : 1];
        V3 CS[SPLIT ? 1 : NC];
        float V[NV];
#define SDFK_RCGET(r) (SPLIT ? V3{CX[SPLIT ? (r) : 0], CY[SPLIT ? (r) : 0], CZ[SPLIT ? (r) : 0]} : CS[SPLIT ? 0 : (r)])
#define SDFK_RCSET(r, q)                                                                             \
    do {                                                                                             \
        const V3 q_ = (q);                                                                           \
        if constexpr (SPLIT) { CX[SPLIT ? (r) : 0] = q_.x; CY[SPLIT ? (r) : 0] = q_.y; CZ[SPLIT ? (r) : 0] = q_.z; } \
        else CS[SPLIT ? 0 : (r)] = q_;                                                               \
    } while (0)
        SDFK_RCSET(0, p0);
        for (int pc = 0; pc < n_instr; ++pc) {
            const uint2 ins = code[pc];                         // wave-uniform: scalar loads
            const unsigned op = ins.x & 255u, a = (ins.x >> 8) & 255u, b = (ins.x >> 16) & 255u, c = ins.x >> 24;
            const float* __restrict__ P = prm + ins.y;
            switch (op) {
#define SDFK_REXEC_C_C(F) SDFK_RCSET(a, F(SDFK_RCGET(b), P, tab, (int)c))
#define SDFK_REXEC_V_C(F) V[a] = F(SDFK_RCGET(b), P, tab)
#define SDFK_REXEC_V_V(F) V[a] = F(V[b], P)
#define SDFK_REXEC_V_VV(F) V[a] = F(V[b], V[c], P)
#define SDFK_OP(NAME, KIND, NP, FUNC) \
    case SDFK_OP_##NAME:              \
        SDFK_REXEC_##KIND(FUNC);      \
        break;
#include "sdfk_ops.def"
#undef SDFK_OP
                default:                                        // (V_FIELD: refused on the host, sdfk_program_rays_check)
                    break;
            }
        }
        return V[result_reg];
#undef SDFK_REXEC_C_C
#undef SDFK_REXEC_V_C
#undef SDFK_REXEC_V_V
#undef SDFK_REXEC_V_VV
#undef SDFK_RCGET
#undef SDFK_RCSET
    }
};

template <int NC, int NV, typename SRC>
__global__ __launch_bounds__(SDFK_RAY_BLOCK) void sdfk_rays_interp_kernel(const uint2* __restrict__ code, int n_instr,
                                                                         const float* __restrict__ prm,
                                                                         const float* __restrict__ tab, int result_reg,
                                                                         SRC src, sdfk_rayopts opts, float* __restrict__ out_t,
                                                                         unsigned char* __restrict__ out_status,
                                                                         int* __restrict__ out_steps,
                                                                         float* __restrict__ out_n, long long nstride) {
    const SdfkInterpField<NC, NV> field = {code, n_instr, prm, tab, result_reg};
    sdfk_trace(src, field, opts, out_t, out_status, out_steps, out_n, nstride);
}

// The span march (sdfk_trace_spans) around the same field object: every crossing and the chord instead of the first hit.
template <int NC, int NV, typename SRC>
__global__ __launch_bounds__(SDFK_RAY_BLOCK) void sdfk_spans_interp_kernel(const uint2* __restrict__ code, int n_instr,
                                                                          const float* __restrict__ prm,
                                                                          const float* __restrict__ tab, int result_reg,
                                                                          SRC src, sdfk_rayopts opts, int max_crossings,
                                                                          float* __restrict__ out_chord, int* __restrict__ out_count,
                                                                          unsigned char* __restrict__ out_status,
                                                                          int* __restrict__ out_steps,
                                                                          float* __restrict__ out_cross, long long cstride) {
    const SdfkInterpField<NC, NV> field = {code, n_instr, prm, tab, result_reg};
    sdfk_trace_spans(src, field, opts, max_crossings, out_chord, out_count, out_status, out_steps, out_cross, cstride);
}

// ---- host side ----------------------------------------------------------------------------------
extern "C" int sdfk_program_rays_check(sdfk_program* p, int* first_bad_op) {
    if (!p) return fail(-1, "null program");
    if (first_bad_op) *first_bad_op = -1;
    const size_t n_instr = p->code.size() / 2;
    for (size_t i = 0; i < n_instr; ++i) {
        const unsigned op = p->code[2 * i] & 255u;
        if (op == SDFK_OP_V_FIELD) {
            if (first_bad_op) *first_bad_op = (int)i;
            char buf[160];
            snprintf(buf, sizeof buf, "instruction %zu (%s): an auxiliary field exists on a grid only, not along rays", i,
                     g_ops[op].name);
            g_err = buf;
            return 1;
        }
    }
    if (p->n_aux > 0) {
        g_err = "the program reads auxiliary fields (staged evaluation)";
        return 1;
    }
    return 0;
}

static int rays_options(const char* who, float t_min, float t_max, float eps, float cone, float inv_lipschitz,
                        int max_steps, sdfk_rayopts* o) {
    const std::string w = who;
    if (!std::isfinite(t_min) || !std::isfinite(t_max)) return fail(-1, w + ": t_min and t_max must be finite");
    if (t_max < t_min) return fail(-1, w + ": t_max < t_min");
    if (!std::isfinite(inv_lipschitz) || !(inv_lipschitz > 0.0f))
        return fail(-1, w + ": the Lipschitz bound must be finite and positive");
    if (max_steps <= 0) return fail(-1, w + ": max_steps must be at least 1");
    if (!(eps >= 0.0f) || !(cone >= 0.0f) || !std::isfinite(eps) || !std::isfinite(cone))
        return fail(-1, w + ": eps and cone must be finite and not negative");
    *o = {t_min, t_max, eps, cone, inv_lipschitz, max_steps};
    return 0;
}

// test aid: what the culled ray kernels of a -DSDFK_DEBUG_RAYSTATS=1 build counted (sdfk_debug_rays_stats). One buffer of
// 8 counters per process; a launch that counts is synchronised and read back at once.
static std::atomic<bool> g_rays_stats_on{false};
static std::mutex g_rays_stats_mu;
static long long g_rays_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
extern "C" void sdfk_debug_rays_stats(int enable, long long* out8) {
    g_rays_stats_on.store(enable != 0);
    if (out8) {
        std::lock_guard<std::mutex> lk(g_rays_stats_mu);
        for (int i = 0; i < 8; ++i) out8[i] = g_rays_stats[i];
        for (int i = 0; i < 8; ++i) g_rays_stats[i] = 0;
    }
}
static int rays_stats_buffer(unsigned long long** out, hipStream_t stream) {
    unsigned long long* b = nullptr;
    HIPCHK(hipMalloc(&b, 8 * sizeof(unsigned long long)));
    if (hipMemsetAsync(b, 0, 8 * sizeof(unsigned long long), stream) != hipSuccess) {   // (ordered with the launch that counts)
        (void)hipFree(b);
        return fail(-2, "sdfk_debug_rays_stats: hipMemsetAsync failed");
    }
    *out = b;
    return 0;
}
static int rays_stats_collect(unsigned long long* b, hipStream_t stream) {
    unsigned long long h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    hipError_t e = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = hipMemcpy(h, b, sizeof h, hipMemcpyDeviceToHost);
    (void)hipFree(b);
    if (e != hipSuccess) return fail(-2, std::string("sdfk_debug_rays_stats: ") + hipGetErrorString(e));
    std::lock_guard<std::mutex> lk(g_rays_stats_mu);
    for (int i = 0; i < 8; ++i) g_rays_stats[i] += (long long)h[i];
    return 0;
}

// array rays (cam == nullptr) or camera rays; `count` = rays (array) or pixels (camera)
static int rays_run(const char* who, sdfk_program* p, const SdfkRaysArray* arr, const sdfk_camera* cam, long long count,
                    const sdfk_rayopts& opts, float* d_t, unsigned char* d_status, int* d_steps, float* d_normals,
                    long long nstride, void* stream_, int mode) {
    const std::string w = who;
    if (!d_t || !d_status || !d_steps) return fail(-1, w + ": null output pointer");
    if (d_normals && nstride < count) return fail(-1, w + ": normal row stride smaller than the ray count");
    int bad = -1;
    const int chk = sdfk_program_rays_check(p, &bad);
    if (chk) return fail(chk < 0 ? chk : -3, w + ": " + g_err);
    if (count == 0) return 0;
    if (mode == SDFK_MODE_AUTO) mode = g_default_mode;
    LaunchCtx x;
    int rc = launch_ctx(p, stream_, &x);
    if (rc) return rc;
    hipStream_t stream = x.stream;
    unsigned blocks;
    if (cam) {
        const long long tiles = (long long)((cam->width + 7) / 8) * ((cam->height + 7) / 8);
        blocks = (unsigned)((tiles + SDFK_RAY_BLOCK / 64 - 1) / (SDFK_RAY_BLOCK / 64));
    } else {
        blocks = (unsigned)((count + SDFK_RAY_BLOCK - 1) / SDFK_RAY_BLOCK);
    }
    std::shared_ptr<SpecModule> sk;                            // (a failed build falls back in AUTO only)
    rc = pick_kernel(p, x.device, SDFK_FL_RAYS, 0, mode, mode == SDFK_MODE_AUTO, "ray kernel", false, &sk);
    if (rc) return rc;
    const float* prm = x.prm;
    const float* tab = x.tab;
    sdfk_rayopts o = opts;
    if (sk) {
        // the culled pair (long chains only) unless the caller asked for the kernel without culling; one more argument,
        // the counters of the statistics build (null otherwise)
        const bool cull = mode != SDFK_MODE_NOCULL && sk->fn[2] && sk->fn[3];
        unsigned long long* stats = nullptr;
        if (cull && g_rays_stats_on.load()) {
            rc = rays_stats_buffer(&stats, stream);
            if (rc) return rc;
        }
        sdfk_camera c;
        SdfkRaysArray a;
        void* src = cam ? (void*)&c : (void*)&a;
        if (cam) c = *cam;
        else a = *arr;
        void* args[] = {&prm, &tab, src, &o, &d_t, &d_status, &d_steps, &d_normals, &nstride, &stats};
        HIPCHK(hipModuleLaunchKernel(sk->fn[(cull ? 2 : 0) + (cam ? 1 : 0)], blocks, 1, 1, SDFK_RAY_BLOCK, 1, 1, 0, stream, args,
                                     nullptr));
        if (stats) {
            rc = rays_stats_collect(stats, stream);
            if (rc) return rc;
        }
        return 0;
    }
    auto launch = [&](auto src) {
        using SRC = decltype(src);
#define SDFK_RAYS_GO(NC, NV) hipLaunchKernelGGL((sdfk_rays_interp_kernel<NC, NV, SRC>), dim3(blocks), dim3(SDFK_RAY_BLOCK), 0, stream, \
                                                x.d->d_code, x.n_instr, prm, tab, x.result_reg, src, o, d_t, d_status, d_steps, d_normals, nstride)
        SDFK_REGFILE(p, SDFK_NC, SDFK_NV, SDFK_RAYS_GO);
#undef SDFK_RAYS_GO
    };
    if (cam) launch(SdfkRaysCamera{*cam});
    else launch(*arr);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sdfk_trace_rays_device(sdfk_program* p, const float* d_origins, int64_t origin_stride,
                                      const float* d_directions, int64_t direction_stride, int64_t n, float t_min,
                                      float t_max, float eps, float cone, float inv_lipschitz, int max_steps, float* d_t,
                                      unsigned char* d_status, int* d_steps, float* d_normals, int64_t normal_stride,
                                      void* stream, int mode) {
    if (!p) return fail(-1, "null program");
    if (n < 0) return fail(-1, "sdfk_trace_rays_device: negative ray count");
    if (n > 0 && (!d_origins || !d_directions)) return fail(-1, "sdfk_trace_rays_device: null ray pointer");
    if (origin_stride < n || direction_stride < n)
        return fail(-1, "sdfk_trace_rays_device: row stride smaller than the ray count");
    sdfk_rayopts o;
    int rc = rays_options("sdfk_trace_rays_device", t_min, t_max, eps, cone, inv_lipschitz, max_steps, &o);
    if (rc) return rc;
    SdfkRaysArray a = {d_origins, (long long)origin_stride, d_directions, (long long)direction_stride, (long long)n};
    return rays_run("sdfk_trace_rays_device", p, &a, nullptr, n, o, d_t, d_status, d_steps, d_normals,
                    (long long)normal_stride, stream, mode);
}

extern "C" int sdfk_trace_camera_device(sdfk_program* p, const float* camera, int width, int height, int orthographic,
                                        float t_min, float t_max, float eps, float cone, float inv_lipschitz, int max_steps,
                                        float* d_t, unsigned char* d_status, int* d_steps, float* d_normals,
                                        int64_t normal_stride, void* stream, int mode) {
    if (!p) return fail(-1, "null program");
    if (!camera) return fail(-1, "sdfk_trace_camera_device: null camera");
    if (width < 0 || height < 0 || width > 32768 || height > 32768)
        return fail(-1, "sdfk_trace_camera_device: image sizes from 0 to 32768");
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(camera[i])) return fail(-1, "sdfk_trace_camera_device: the camera record is not finite");
    sdfk_rayopts o;
    int rc = rays_options("sdfk_trace_camera_device", t_min, t_max, eps, cone, inv_lipschitz, max_steps, &o);
    if (rc) return rc;
    sdfk_camera c;
    for (int i = 0; i < 3; ++i) c.eye[i] = camera[i], c.fwd[i] = camera[3 + i], c.du[i] = camera[6 + i], c.dv[i] = camera[9 + i];
    c.inv_w = width ? 1.0f / (float)width : 0.0f;
    c.inv_h = height ? 1.0f / (float)height : 0.0f;
    c.width = width, c.height = height, c.ortho = orthographic ? 1 : 0;
    return rays_run("sdfk_trace_camera_device", p, nullptr, &c, (long long)width * height, o, d_t, d_status, d_steps,
                    d_normals, (long long)normal_stride, stream, mode);
}

// ---- spans: every crossing and the chord (sdfk_trace_spans) --------------------------------------------------------------
// array rays (cam == nullptr) or camera rays, as rays_run; the kernel follows pick_kernel exactly as there
static int spans_run(const char* who, sdfk_program* p, const SdfkRaysArray* arr, const sdfk_camera* cam, long long count,
                     const sdfk_rayopts& opts, float* d_chord, int* d_count, unsigned char* d_status, int* d_steps,
                     float* d_cross, long long cstride, int max_crossings, void* stream_, int mode) {
    const std::string w = who;
    if (!d_chord || !d_count || !d_status || !d_steps) return fail(-1, w + ": null output pointer");
    if (max_crossings < 0 || max_crossings > SDFK_SPAN_MAX_CROSSINGS)
        return fail(-1, w + ": max_crossings from 0 to " + std::to_string(SDFK_SPAN_MAX_CROSSINGS));
    if (d_cross && max_crossings > 0 && cstride < count) return fail(-1, w + ": crossing row stride smaller than the ray count");
    int K = d_cross ? max_crossings : 0;                       // (no array: the crossings are counted and not stored)
    int bad = -1;
    const int chk = sdfk_program_rays_check(p, &bad);
    if (chk) return fail(chk < 0 ? chk : -3, w + ": " + g_err);
    if (count == 0) return 0;
    if (mode == SDFK_MODE_AUTO) mode = g_default_mode;
    LaunchCtx x;
    int rc = launch_ctx(p, stream_, &x);
    if (rc) return rc;
    hipStream_t stream = x.stream;
    unsigned blocks;
    if (cam) {
        const long long tiles = (long long)((cam->width + 7) / 8) * ((cam->height + 7) / 8);
        blocks = (unsigned)((tiles + SDFK_RAY_BLOCK / 64 - 1) / (SDFK_RAY_BLOCK / 64));
    } else {
        blocks = (unsigned)((count + SDFK_RAY_BLOCK - 1) / SDFK_RAY_BLOCK);
    }
    std::shared_ptr<SpecModule> sk;                            // (a failed build falls back in AUTO only)
    rc = pick_kernel(p, x.device, SDFK_FL_SPANS, 0, mode, mode == SDFK_MODE_AUTO, "span kernel", false, &sk);
    if (rc) return rc;
    const float* prm = x.prm;
    const float* tab = x.tab;
    sdfk_rayopts o = opts;
    if (sk) {
        const bool cull = mode != SDFK_MODE_NOCULL && sk->fn[2] && sk->fn[3];   // the culled pair: long chains only
        sdfk_camera c;
        SdfkRaysArray a;
        void* src = cam ? (void*)&c : (void*)&a;
        if (cam) c = *cam;
        else a = *arr;
        void* args[] = {&prm, &tab, src, &o, &K, &d_chord, &d_count, &d_status, &d_steps, &d_cross, &cstride};
        HIPCHK(hipModuleLaunchKernel(sk->fn[(cull ? 2 : 0) + (cam ? 1 : 0)], blocks, 1, 1, SDFK_RAY_BLOCK, 1, 1, 0, stream, args,
                                     nullptr));
        return 0;
    }
    auto launch = [&](auto src) {
        using SRC = decltype(src);
#define SDFK_SPANS_GO(NC, NV) hipLaunchKernelGGL((sdfk_spans_interp_kernel<NC, NV, SRC>), dim3(blocks), dim3(SDFK_RAY_BLOCK), 0, stream, \
                                                 x.d->d_code, x.n_instr, prm, tab, x.result_reg, src, o, K, d_chord, d_count, d_status, d_steps, d_cross, cstride)
        SDFK_REGFILE(p, SDFK_NC, SDFK_NV, SDFK_SPANS_GO);
#undef SDFK_SPANS_GO
    };
    if (cam) launch(SdfkRaysCamera{*cam});
    else launch(*arr);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sdfk_span_rays_device(sdfk_program* p, const float* d_origins, int64_t origin_stride, const float* d_directions,
                                     int64_t direction_stride, int64_t n, float t_min, float t_max, float eps, float cone,
                                     float inv_lipschitz, int max_steps, float* d_chord, int* d_count, unsigned char* d_status,
                                     int* d_steps, float* d_crossings, int64_t crossing_stride, int max_crossings, void* stream,
                                     int mode) {
    if (!p) return fail(-1, "null program");
    if (n < 0) return fail(-1, "sdfk_span_rays_device: negative ray count");
    if (n > 0 && (!d_origins || !d_directions)) return fail(-1, "sdfk_span_rays_device: null ray pointer");
    if (origin_stride < n || direction_stride < n)
        return fail(-1, "sdfk_span_rays_device: row stride smaller than the ray count");
    sdfk_rayopts o;
    int rc = rays_options("sdfk_span_rays_device", t_min, t_max, eps, cone, inv_lipschitz, max_steps, &o);
    if (rc) return rc;
    SdfkRaysArray a = {d_origins, (long long)origin_stride, d_directions, (long long)direction_stride, (long long)n};
    return spans_run("sdfk_span_rays_device", p, &a, nullptr, n, o, d_chord, d_count, d_status, d_steps, d_crossings,
                     (long long)crossing_stride, max_crossings, stream, mode);
}

extern "C" int sdfk_span_camera_device(sdfk_program* p, const float* camera, int width, int height, int orthographic,
                                       float t_min, float t_max, float eps, float cone, float inv_lipschitz, int max_steps,
                                       float* d_chord, int* d_count, unsigned char* d_status, int* d_steps, float* d_crossings,
                                       int64_t crossing_stride, int max_crossings, void* stream, int mode) {
    if (!p) return fail(-1, "null program");
    if (!camera) return fail(-1, "sdfk_span_camera_device: null camera");
    if (width < 0 || height < 0 || width > 32768 || height > 32768)
        return fail(-1, "sdfk_span_camera_device: image sizes from 0 to 32768");
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(camera[i])) return fail(-1, "sdfk_span_camera_device: the camera record is not finite");
    sdfk_rayopts o;
    int rc = rays_options("sdfk_span_camera_device", t_min, t_max, eps, cone, inv_lipschitz, max_steps, &o);
    if (rc) return rc;
    sdfk_camera c;
    for (int i = 0; i < 3; ++i) c.eye[i] = camera[i], c.fwd[i] = camera[3 + i], c.du[i] = camera[6 + i], c.dv[i] = camera[9 + i];
    c.inv_w = width ? 1.0f / (float)width : 0.0f;
    c.inv_h = height ? 1.0f / (float)height : 0.0f;
    c.width = width, c.height = height, c.ortho = orthographic ? 1 : 0;
    return spans_run("sdfk_span_camera_device", p, nullptr, &c, (long long)width * height, o, d_chord, d_count, d_status,
                     d_steps, d_crossings, (long long)crossing_stride, max_crossings, stream, mode);
}
