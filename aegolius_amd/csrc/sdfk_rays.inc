// sdfk_rays.inc — sphere tracing of a program (included at the end of sdfk.hip; the loops themselves: sdfk_raydev.h).
//
//   * sdfk_march_interp_kernel<NC, NV, SRC, OUT> : the interpreter's register machine as a __device__ evaluation of ONE
//     point (SdfkInterpField, sdfk_interpfield.h) called from the marching loop that OUT selects: SdfkHitOut the first hit,
//     SdfkSpanOut the march that goes on through the surface (every crossing, the chord), SdfkVisOut the visibility of a
//     segment and SdfkAoOut ambient occlusion (the secondary marches: array rays only). One ray per lane; the code words
//     are wave-uniform (scalar loads) because the loop's trip count is. SRC = SdfkRaysArray (two (3, n) arrays) or
//     SdfkRaysCamera (rays generated from the camera record, one 8 x 8 pixel tile per wave). Register files as in
//     sdfk_interp_kernel, and with the same outcome as its one-point-per-lane instantiations (compiler's resource remarks,
//     all four first-hit instances: 57 VGPRs, 8 waves per SIMD): the small coordinate file stays in VGPRs and its three
//     value registers, indexed by the wave-uniform operand fields, take 16 bytes of scratch per lane
//     (sdfk_interp_kernel<1, 2, 3>: 16 as well); the full file takes 128.
//   * the specialised flavours (SDFK_FL_RAYS, SDFK_FL_SPANS, SDFK_FL_SECONDARY, sdfk_codegen.cpp) wrap the generated sdfk_point<float> in the
//     same loops; long hard unions (chain mode) get a second pair of kernels there that folds the chain over per-wave
//     survivor lists in LDS (sdfk_raycull.h) — what SPECIALIZED / AUTO launch, NOCULL the plain pair; same bits.
//   * the host side is one path for all marches: an entry point fills a MarchRequest, march_run picks and launches.
// Outputs per ray, first hit: t (fp32), status (1 byte: 0 miss, 1 hit, 2 step limit), steps (int32), optionally the
// stencil normal (three strided rows). Plain vector stores, written once; no atomics, no LDS.
#include "sdfk_interpfield.h"
#include "sdfk_raydev.h"

template <int NC, int NV, typename SRC, typename OUT>
__global__ __launch_bounds__(SDFK_RAY_BLOCK) void sdfk_march_interp_kernel(const uint2* __restrict__ code, int n_instr,
                                                                          const float* __restrict__ prm,
                                                                          const float* __restrict__ tab, int result_reg,
                                                                          SRC src, sdfk_rayopts opts, OUT out) {
    const SdfkInterpField<NC, NV> field = {code, n_instr, prm, tab, result_reg};
    sdfk_march(src, field, opts, out);
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

// ---- one request, one runner ---------------------------------------------------------------------------------------------
struct MarchRequest {
    const char* who;                                  // the entry point, for messages
    sdfk_program* p;
    std::variant<SdfkRaysArray, sdfk_camera> src;     // array rays (count = rays), or a parsed camera (count = pixels)
    long long count;
    sdfk_rayopts opts;
    std::variant<SdfkHitOut, SdfkSpanOut, SdfkVisOut, SdfkAoOut> out;   // the output record, which also says which march
    void* stream;
    int mode;
};

// the caller's 12 floats {eye, fwd, du, dv} and the image size -> the kernels' record
static int camera_record(const char* who, const float* camera, int width, int height, int orthographic, sdfk_camera* c) {
    const std::string w = who;
    if (!camera) return fail(-1, w + ": null camera");
    if (width < 0 || height < 0 || width > 32768 || height > 32768) return fail(-1, w + ": image sizes from 0 to 32768");
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(camera[i])) return fail(-1, w + ": the camera record is not finite");
    for (int i = 0; i < 3; ++i)
        c->eye[i] = camera[i], c->fwd[i] = camera[3 + i], c->du[i] = camera[6 + i], c->dv[i] = camera[9 + i];
    c->inv_w = width ? 1.0f / (float)width : 0.0f;
    c->inv_h = height ? 1.0f / (float)height : 0.0f;
    c->width = width, c->height = height, c->ortho = orthographic ? 1 : 0;
    return 0;
}
static int ray_arrays(const char* who, const float* d_origins, int64_t origin_stride, const float* d_directions,
                      int64_t direction_stride, int64_t n, SdfkRaysArray* a) {
    const std::string w = who;
    if (n < 0) return fail(-1, w + ": negative ray count");
    if (n > 0 && (!d_origins || !d_directions)) return fail(-1, w + ": null ray pointer");
    if (origin_stride < n || direction_stride < n) return fail(-1, w + ": row stride smaller than the ray count");
    *a = {d_origins, (long long)origin_stride, d_directions, (long long)direction_stride, (long long)n};
    return 0;
}
static int hit_outputs(const char* who, float* d_t, unsigned char* d_status, int* d_steps, float* d_normals,
                       int64_t normal_stride, long long count, SdfkHitOut* out) {
    const std::string w = who;
    if (!d_t || !d_status || !d_steps) return fail(-1, w + ": null output pointer");
    if (d_normals && normal_stride < count) return fail(-1, w + ": normal row stride smaller than the ray count");
    *out = {d_t, d_status, d_steps, d_normals, (long long)normal_stride};
    return 0;
}
static int span_outputs(const char* who, float* d_chord, int* d_count, unsigned char* d_status, int* d_steps,
                        float* d_crossings, int64_t crossing_stride, int max_crossings, long long count, SdfkSpanOut* out) {
    const std::string w = who;
    if (!d_chord || !d_count || !d_status || !d_steps) return fail(-1, w + ": null output pointer");
    if (max_crossings < 0 || max_crossings > SDFK_SPAN_MAX_CROSSINGS)
        return fail(-1, w + ": max_crossings from 0 to " + std::to_string(SDFK_SPAN_MAX_CROSSINGS));
    if (d_crossings && max_crossings > 0 && crossing_stride < count)
        return fail(-1, w + ": crossing row stride smaller than the ray count");
    // (no array: the crossings are counted and not stored)
    *out = {d_chord, d_count, d_status, d_steps, d_crossings, (long long)crossing_stride, d_crossings ? max_crossings : 0};
    return 0;
}

static int vis_outputs(const char* who, float softness, const float* d_limits, float* d_vis, unsigned char* d_status,
                       int* d_steps, SdfkVisOut* out) {
    const std::string w = who;
    if (!std::isfinite(softness) || !(softness >= 0.0f)) return fail(-1, w + ": softness must be finite and not negative");
    if (!d_vis || !d_status || !d_steps) return fail(-1, w + ": null output pointer");
    *out = {softness, d_limits, d_vis, d_status, d_steps};
    return 0;
}

// What march_run asks of an output record: the flavour that holds its kernels and its name in messages, which of the
// flavour's two kernels runs it (first hit and spans: the camera one; the secondary flavour: the occlusion one), whether
// the march has a camera source at all, and its kernel arguments in the order of its SDFK_*_PARAMS.
struct MarchKind {
    int flavour;
    const char* what;
    bool second, camera;
};
static MarchKind march_kind(const SdfkHitOut&, bool cam) { return {SDFK_FL_RAYS, "ray kernel", cam, true}; }
static MarchKind march_kind(const SdfkSpanOut&, bool cam) { return {SDFK_FL_SPANS, "span kernel", cam, true}; }
static MarchKind march_kind(const SdfkVisOut&, bool) { return {SDFK_FL_SECONDARY, "visibility kernel", false, false}; }
static MarchKind march_kind(const SdfkAoOut&, bool) { return {SDFK_FL_SECONDARY, "occlusion kernel", true, false}; }
static int march_args(SdfkHitOut& h, void** a) {
    int n = 0;
    for (void* x : {(void*)&h.t, (void*)&h.status, (void*)&h.steps, (void*)&h.n, (void*)&h.nstride}) a[n++] = x;
    return n;
}
static int march_args(SdfkSpanOut& s, void** a) {
    int n = 0;
    for (void* x : {(void*)&s.max_crossings, (void*)&s.chord, (void*)&s.count, (void*)&s.status, (void*)&s.steps, (void*)&s.cross,
                    (void*)&s.cstride})
        a[n++] = x;
    return n;
}
static int march_args(SdfkVisOut& v, void** a) {
    int n = 0;
    for (void* x : {(void*)&v.softness, (void*)&v.limits, (void*)&v.vis, (void*)&v.status, (void*)&v.steps}) a[n++] = x;
    return n;
}
static int march_args(SdfkAoOut& o, void** a) {
    int n = 0;
    for (void* x : {(void*)&o.inv_m, (void*)&o.inv_radius, (void*)&o.strength, (void*)&o.ao}) a[n++] = x;
    return n;
}

// The program's check, the kernel that serves the call (pick_kernel) and its launch. The marches differ in what march_kind
// says of their record, in their kernel arguments and in the counters of the statistics build, which only the culled
// first-hit kernels feed.
static int march_run(const MarchRequest& r) {
    int bad = -1;
    const int chk = sdfk_program_rays_check(r.p, &bad);
    if (chk) return fail(chk < 0 ? chk : -3, std::string(r.who) + ": " + g_err);
    if (r.count == 0) return 0;
    const int mode = r.mode == SDFK_MODE_AUTO ? g_default_mode : r.mode;
    LaunchCtx x;
    int rc = launch_ctx(r.p, r.stream, &x);
    if (rc) return rc;
    hipStream_t stream = x.stream;
    const sdfk_camera* cam = std::get_if<sdfk_camera>(&r.src);
    const MarchKind kind = std::visit([&](const auto& o) { return march_kind(o, cam != nullptr); }, r.out);
    if (cam && !kind.camera) return fail(-1, std::string(r.who) + ": this march has no camera source");
    unsigned blocks;
    if (cam) {
        const long long tiles = (long long)((cam->width + 7) / 8) * ((cam->height + 7) / 8);
        blocks = (unsigned)((tiles + SDFK_RAY_BLOCK / 64 - 1) / (SDFK_RAY_BLOCK / 64));
    } else {
        blocks = (unsigned)((r.count + SDFK_RAY_BLOCK - 1) / SDFK_RAY_BLOCK);
    }
    std::shared_ptr<SpecModule> sk;                            // (a failed build falls back in AUTO only)
    rc = pick_kernel(r.p, x.device, kind.flavour, 0, mode, mode == SDFK_MODE_AUTO, kind.what, false, &sk);
    if (rc) return rc;
    const float* prm = x.prm;
    const float* tab = x.tab;
    if (sk) {
        // the culled pair (long chains only) unless the caller asked for the kernel without culling
        const bool cull = mode != SDFK_MODE_NOCULL && sk->fn[2] && sk->fn[3];
        unsigned long long* stats = nullptr;
        if (cull && kind.flavour == SDFK_FL_RAYS && g_rays_stats_on.load()) {
            rc = rays_stats_buffer(&stats, stream);
            if (rc) return rc;
        }
        // (PRM, TAB, source, opts, the march's outputs in the order of its SDFK_*_PARAMS, STATS)
        auto src = r.src;
        auto out = r.out;
        sdfk_rayopts opts = r.opts;
        void* args[12] = {&prm, &tab, std::visit([](auto& s) { return (void*)&s; }, src), &opts};
        int n = 4;
        n += std::visit([&](auto& o) { return march_args(o, args + n); }, out);
        args[n++] = &stats;
        HIPCHK(hipModuleLaunchKernel(sk->fn[(cull ? 2 : 0) + (kind.second ? 1 : 0)], blocks, 1, 1, SDFK_RAY_BLOCK, 1, 1, 0, stream, args,
                                     nullptr));
        if (stats) {
            rc = rays_stats_collect(stats, stream);
            if (rc) return rc;
        }
        return 0;
    }
    auto launch = [&](auto src, auto out) {
        using SRC = decltype(src);
        using OUT = decltype(out);
#define SDFK_MARCH_GO(NC, NV) hipLaunchKernelGGL((sdfk_march_interp_kernel<NC, NV, SRC, OUT>), dim3(blocks), dim3(SDFK_RAY_BLOCK), 0, stream, \
                                                 x.d->d_code, x.n_instr, prm, tab, x.result_reg, src, r.opts, out)
        SDFK_REGFILE(r.p, SDFK_NC, SDFK_NV, SDFK_MARCH_GO);
#undef SDFK_MARCH_GO
    };
    std::visit([&](auto out) {
        // (a march without a camera source has no camera instance of the interpreter kernel either)
        if constexpr (std::is_same_v<decltype(out), SdfkHitOut> || std::is_same_v<decltype(out), SdfkSpanOut>) {
            if (cam) {
                launch(SdfkRaysCamera{*cam}, out);
                return;
            }
        }
        launch(std::get<SdfkRaysArray>(r.src), out);
    }, r.out);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- the entry points: each fills a request, in the order its checks report ------------------------------------------------
extern "C" int sdfk_trace_rays_device(sdfk_program* p, const float* d_origins, int64_t origin_stride,
                                      const float* d_directions, int64_t direction_stride, int64_t n, float t_min,
                                      float t_max, float eps, float cone, float inv_lipschitz, int max_steps, float* d_t,
                                      unsigned char* d_status, int* d_steps, float* d_normals, int64_t normal_stride,
                                      void* stream, int mode) {
    if (!p) return fail(-1, "null program");
    MarchRequest r = {"sdfk_trace_rays_device", p, SdfkRaysArray{}, (long long)n, {}, SdfkHitOut{}, stream, mode};
    int rc = ray_arrays(r.who, d_origins, origin_stride, d_directions, direction_stride, n, &std::get<SdfkRaysArray>(r.src));
    if (!rc) rc = rays_options(r.who, t_min, t_max, eps, cone, inv_lipschitz, max_steps, &r.opts);
    if (!rc) rc = hit_outputs(r.who, d_t, d_status, d_steps, d_normals, normal_stride, r.count, &std::get<SdfkHitOut>(r.out));
    return rc ? rc : march_run(r);
}

extern "C" int sdfk_trace_camera_device(sdfk_program* p, const float* camera, int width, int height, int orthographic,
                                        float t_min, float t_max, float eps, float cone, float inv_lipschitz, int max_steps,
                                        float* d_t, unsigned char* d_status, int* d_steps, float* d_normals,
                                        int64_t normal_stride, void* stream, int mode) {
    if (!p) return fail(-1, "null program");
    MarchRequest r = {"sdfk_trace_camera_device", p, sdfk_camera{}, (long long)width * height, {}, SdfkHitOut{}, stream, mode};
    int rc = camera_record(r.who, camera, width, height, orthographic, &std::get<sdfk_camera>(r.src));
    if (!rc) rc = rays_options(r.who, t_min, t_max, eps, cone, inv_lipschitz, max_steps, &r.opts);
    if (!rc) rc = hit_outputs(r.who, d_t, d_status, d_steps, d_normals, normal_stride, r.count, &std::get<SdfkHitOut>(r.out));
    return rc ? rc : march_run(r);
}

extern "C" int sdfk_span_rays_device(sdfk_program* p, const float* d_origins, int64_t origin_stride, const float* d_directions,
                                     int64_t direction_stride, int64_t n, float t_min, float t_max, float eps, float cone,
                                     float inv_lipschitz, int max_steps, float* d_chord, int* d_count, unsigned char* d_status,
                                     int* d_steps, float* d_crossings, int64_t crossing_stride, int max_crossings, void* stream,
                                     int mode) {
    if (!p) return fail(-1, "null program");
    MarchRequest r = {"sdfk_span_rays_device", p, SdfkRaysArray{}, (long long)n, {}, SdfkSpanOut{}, stream, mode};
    int rc = ray_arrays(r.who, d_origins, origin_stride, d_directions, direction_stride, n, &std::get<SdfkRaysArray>(r.src));
    if (!rc) rc = rays_options(r.who, t_min, t_max, eps, cone, inv_lipschitz, max_steps, &r.opts);
    if (!rc) rc = span_outputs(r.who, d_chord, d_count, d_status, d_steps, d_crossings, crossing_stride, max_crossings, r.count, &std::get<SdfkSpanOut>(r.out));
    return rc ? rc : march_run(r);
}

extern "C" int sdfk_span_camera_device(sdfk_program* p, const float* camera, int width, int height, int orthographic,
                                       float t_min, float t_max, float eps, float cone, float inv_lipschitz, int max_steps,
                                       float* d_chord, int* d_count, unsigned char* d_status, int* d_steps, float* d_crossings,
                                       int64_t crossing_stride, int max_crossings, void* stream, int mode) {
    if (!p) return fail(-1, "null program");
    MarchRequest r = {"sdfk_span_camera_device", p, sdfk_camera{}, (long long)width * height, {}, SdfkSpanOut{}, stream, mode};
    int rc = camera_record(r.who, camera, width, height, orthographic, &std::get<sdfk_camera>(r.src));
    if (!rc) rc = rays_options(r.who, t_min, t_max, eps, cone, inv_lipschitz, max_steps, &r.opts);
    if (!rc) rc = span_outputs(r.who, d_chord, d_count, d_status, d_steps, d_crossings, crossing_stride, max_crossings, r.count, &std::get<SdfkSpanOut>(r.out));
    return rc ? rc : march_run(r);
}

// ---- the secondary marches: array rays only ------------------------------------------------------------------------------------
extern "C" int sdfk_visibility_rays_device(sdfk_program* p, const float* d_origins, int64_t origin_stride,
                                           const float* d_directions, int64_t direction_stride, int64_t n, float t_min,
                                           float t_max, float eps, float cone, float inv_lipschitz, int max_steps, float softness,
                                           const float* d_limits, float* d_vis, unsigned char* d_status, int* d_steps,
                                           void* stream, int mode) {
    if (!p) return fail(-1, "null program");
    MarchRequest r = {"sdfk_visibility_rays_device", p, SdfkRaysArray{}, (long long)n, {}, SdfkVisOut{}, stream, mode};
    int rc = ray_arrays(r.who, d_origins, origin_stride, d_directions, direction_stride, n, &std::get<SdfkRaysArray>(r.src));
    if (!rc) rc = rays_options(r.who, t_min, t_max, eps, cone, inv_lipschitz, max_steps, &r.opts);
    if (!rc && !(t_min >= 0.0f)) rc = fail(-1, std::string(r.who) + ": t_min must not be negative");
    if (!rc) rc = vis_outputs(r.who, softness, d_limits, d_vis, d_status, d_steps, &std::get<SdfkVisOut>(r.out));
    return rc ? rc : march_run(r);
}

extern "C" int sdfk_occlusion_rays_device(sdfk_program* p, const float* d_points, int64_t point_stride, const float* d_normals,
                                          int64_t normal_stride, int64_t n, float radius, int samples, float strength,
                                          float inv_lipschitz, float* d_ao, void* stream, int mode) {
    if (!p) return fail(-1, "null program");
    MarchRequest r = {"sdfk_occlusion_rays_device", p, SdfkRaysArray{}, (long long)n, {}, SdfkAoOut{}, stream, mode};
    const std::string w = r.who;
    int rc = ray_arrays(r.who, d_points, point_stride, d_normals, normal_stride, n, &std::get<SdfkRaysArray>(r.src));
    if (rc) return rc;
    if (!std::isfinite(radius) || !(radius > 0.0f)) return fail(-1, w + ": radius must be finite and positive");
    if (samples < 1 || samples > SDFK_AO_MAX_SAMPLES)
        return fail(-1, w + ": samples from 1 to " + std::to_string(SDFK_AO_MAX_SAMPLES));
    if (!std::isfinite(strength) || !(strength >= 0.0f)) return fail(-1, w + ": strength must be finite and not negative");
    // the options the loop reads: t_max = the radius, max_steps = the samples, 1 / L (t_min, eps and cone play no part)
    rc = rays_options(r.who, 0.0f, radius, 0.0f, 0.0f, inv_lipschitz, samples, &r.opts);
    if (rc) return rc;
    if (!d_ao) return fail(-1, w + ": null output pointer");
    r.out = SdfkAoOut{1.0f / (float)samples, 1.0f / radius, strength, d_ao};
    return march_run(r);
}
