// sdfk_project.inc — Newton projection of points onto a level set (included after sdfk_dual.inc; rules in sdfk_dualdev.h).
//
//   * sdfk_project_kernel<NC, NV, SRC> : sdfk_jvp_kernel's register machine in point mode (K = 3, coordinate tangents
//     e_x, e_y, e_z, parameter tangents zero) inside an iteration loop, one point per lane. Per lane, in fp32:
//         q = p; it = 0
//         loop: (f, g) = program on dual numbers at q            every instruction, wave-uniform
//               if it == 0: start = f
//               r = f - level
//               if !(|r| <= FLT_MAX)  -> NONFINITE, stop
//               if |r| <= tol         -> CONVERGED, stop
//               if it == max_iter     -> MAXITER,   stop
//               g2 = (gx gx + gy gy) + gz gz
//               if !(g2 >= 1e-24)     -> STALLED,   stop          a centre, an axis, a flat map
//               s = relax (r / g2);  q = q - s g;  it += 1
//     A lane that has stopped keeps q, f and g and goes on executing the program with its wave; the wave leaves when no
//     lane is active (the vote of sdfk_raydev.h). The trip count is at most max_iter + 1 <= 256 whatever the input.
//     The tests on r and g2 that a NaN must fail are integer compares: the build has -fno-honor-nans (sdfk_access.h).
// Traffic: 12 B of coordinates in; 12 B (q) + 4 B (value) + 4 B (status, iterations) out, plus 12 B (gradient) and 4 B
// (start) when asked for — 36 B at most, whatever the iteration count.
#define SDFK_PROJECT_CONVERGED 0u
#define SDFK_PROJECT_MAXITER 1u
#define SDFK_PROJECT_STALLED 2u
#define SDFK_PROJECT_NONFINITE 3u
#define SDFK_PROJECT_GMIN2 1e-24f

template <int NC, int NV, typename SRC>
__global__ __launch_bounds__(SDFK_BLOCK) void sdfk_project_kernel(
    const uint2* __restrict__ code, int n_instr, const float* __restrict__ prm, const float* __restrict__ dprm, int ns,
    const float* __restrict__ tab, SRC src, long long n, float level, float tol, int max_iter, float relax,
    float* __restrict__ out_q, long long qstride, float* __restrict__ out_v, float* __restrict__ out_g, long long gstride,
    float* __restrict__ out_start, int* __restrict__ out_info, unsigned* __restrict__ wg_trips, int result_reg) {
    constexpr int K = 3;
    const long long block_base = (long long)sdfk_bx() * SDFK_BLOCK;
    const unsigned lane = sdfk_tx();
    const long long i = block_base + lane;
    if (i >= n) return;
    float Cx[NC], Cy[NC], Cz[NC], Ctx[NC * K], Cty[NC * K], Ctz[NC * K];
    float VV[NV], VT[NV * K];
    V3 q;
    {
        V3 p[1];
        sdfk_load<1>(src, block_base, lane, p);
        q = p[0];
#pragma unroll
        for (int r = 0; r < NC; ++r) {
            Cx[r] = q.x, Cy[r] = q.y, Cz[r] = q.z;
            SDFK_KLOOP {
                Ctx[r * K + k] = (k == 0) ? 1.0f : 0.0f;
                Cty[r * K + k] = (k == 1) ? 1.0f : 0.0f;
                Ctz[r * K + k] = (k == 2) ? 1.0f : 0.0f;
            }
        }
#pragma unroll
        for (int r = 0; r < NV; ++r) {
            VV[r] = 0.0f;
            SDFK_KLOOP VT[r * K + k] = 0.0f;
        }
    }
    float f = 0.0f, gx = 0.0f, gy = 0.0f, gz = 0.0f, start = 0.0f;
    unsigned status = SDFK_PROJECT_MAXITER;
    int it = 0, trips = 0;
    bool active = true;
    for (int trip = 0; trip <= max_iter; ++trip) {       // an active lane stops or steps on every trip: it == trip
        // register 0 is the input point; every other register is written before it is read (validate())
        Cx[0] = q.x, Cy[0] = q.y, Cz[0] = q.z;
        SDFK_KLOOP {
            Ctx[k] = (k == 0) ? 1.0f : 0.0f;
            Cty[k] = (k == 1) ? 1.0f : 0.0f;
            Ctz[k] = (k == 2) ? 1.0f : 0.0f;
        }
        for (int pc = 0; pc < n_instr; ++pc) {
            const uint2 ins = code[pc];                     // wave-uniform: scalar loads
            const unsigned op = ins.x & 255u, a = (ins.x >> 8) & 255u, b = (ins.x >> 16) & 255u, c = ins.x >> 24;
            const float* __restrict__ P = prm + ins.y;
            const float* __restrict__ Q = dprm + ins.y;
            switch (op) {
#define SDFK_DUAL_CASE(NAME, KIND, FN) \
    case SDFK_OP_##NAME:               \
        SDFK_DUAL_EXEC_##KIND(FN);     \
        break;
                SDFK_DUAL_TABLE(SDFK_DUAL_CASE)
#undef SDFK_DUAL_CASE
                default:                                    // refused on the host (sdfk_program_jvp_check)
                    break;
            }
        }
        DS<K> r;
        SDFK_VF_GET((unsigned)result_reg, r);
        ++trips;
        if (trip == 0) start = r.v;
        if (active) {
            f = r.v, gx = r.d[0], gy = r.d[1], gz = r.d[2];
            const float res = f - level;
            const float g2 = (gx * gx + gy * gy) + gz * gz;
            const unsigned rb = __builtin_bit_cast(unsigned, res) & 0x7fffffffu, gb = __builtin_bit_cast(unsigned, g2);
            if (rb >= 0x7f800000u) {
                status = SDFK_PROJECT_NONFINITE, active = false;
            } else if (fabsf(res) <= tol) {
                status = SDFK_PROJECT_CONVERGED, active = false;
            } else if (it == max_iter) {
                status = SDFK_PROJECT_MAXITER, active = false;
            } else if (!(gb >= __builtin_bit_cast(unsigned, SDFK_PROJECT_GMIN2) && gb <= 0x7f800000u)) {
                status = SDFK_PROJECT_STALLED, active = false;       // g2 is a sum of squares: its bits order like its value
            } else {
                const float s = relax * (res / g2);
                q.x = q.x - s * gx, q.y = q.y - s * gy, q.z = q.z - s * gz;
                ++it;
            }
        }
        if (!__any(active)) break;
    }
    out_q[i] = q.x, out_q[qstride + i] = q.y, out_q[2 * qstride + i] = q.z;
    out_v[i] = f;
    if (out_g) out_g[i] = gx, out_g[gstride + i] = gy, out_g[2 * gstride + i] = gz;
    if (out_start) out_start[i] = start;
    out_info[i] = (int)(status | ((unsigned)it << 8));
    // evaluations this wave ran (measurement only): its first live lane adds them to the workgroup's counter
    if (wg_trips) {
        const unsigned long long live = __ballot(1);
        if ((lane & 63u) == (unsigned)(__ffsll((long long)live) - 1)) atomicAdd(&wg_trips[sdfk_bx()], (unsigned)trips);
    }
}

// ---- host side ----------------------------------------------------------------------------------
// K = 3 rows of zero parameter tangents for the program on the current device (DevState::d_ptan0), made on first use
static int project_zero_tangents(sdfk_program* p, DevState* d) {
    std::lock_guard<std::mutex> lk(p->mu);
    if (d->d_ptan0) return 0;
    const size_t bytes = std::max<size_t>(3 * p->params.size(), 1) * sizeof(float);
    float* z = nullptr;
    HIPCHK(hipMalloc(&z, bytes));
    const hipError_t e = hipMemset(z, 0, bytes);
    if (e != hipSuccess) {
        (void)hipFree(z);
        HIPCHK(e);
    }
    d->d_ptan0 = z;
    return 0;
}

static int project_points(sdfk_program* p, const float* d_co, int64_t n, int64_t row_stride, float level, float tol,
                          int max_iter, float relax, float* d_q, int64_t q_stride, float* d_value, float* d_grad,
                          int64_t grad_stride, float* d_start, int32_t* d_info, uint32_t* d_wg_trips, void* stream) {
    const char* who = "sdfk_project_points_device: ";
    if (!p) return fail(-1, "null program");
    if (!d_co || !d_q || !d_value || !d_info) return fail(-1, std::string(who) + "null device pointer");
    if (n < 0 || row_stride < n || q_stride < n || (d_grad && grad_stride < n))
        return fail(-1, std::string(who) + "row, point or gradient stride smaller than the point count");
    if (max_iter < 0 || max_iter > 255) return fail(-1, std::string(who) + "max_iter outside 0 .. 255");
    if (!(tol >= 0.0f)) return fail(-1, std::string(who) + "tol must be >= 0");
    if (!std::isfinite(level) || !std::isfinite(relax)) return fail(-1, std::string(who) + "level and relax must be finite");
    if (!(relax > 0.0f && relax <= 1.0f)) return fail(-1, std::string(who) + "relax outside (0, 1]");
    int bad = -1;
    const int chk = sdfk_program_jvp_check(p, &bad);
    if (chk) return fail(chk < 0 ? chk : -3, std::string(who) + g_err);
    if (n == 0) return 0;
    LaunchCtx x;
    int rc = launch_ctx(p, stream, &x);
    if (rc) return rc;
    rc = project_zero_tangents(p, x.d);
    if (rc) return rc;
    const unsigned blocks = (unsigned)((n + SDFK_BLOCK - 1) / SDFK_BLOCK);
    SrcArray src = {d_co, (long long)row_stride};
    const int ns = (int)p->params.size();
#define SDFK_PROJECT_GO(NC, NV)                                                                                            \
    hipLaunchKernelGGL((sdfk_project_kernel<NC, NV, SrcArray>), dim3(blocks), dim3(SDFK_BLOCK), 0, x.stream, x.d->d_code,  \
                       x.n_instr, x.prm, x.d->d_ptan0, ns, x.tab, src, (long long)n, level, tol, max_iter, relax, d_q,     \
                       (long long)q_stride, d_value, d_grad, (long long)grad_stride, d_start, d_info, d_wg_trips,          \
                       x.result_reg)
    SDFK_REGFILE(p, SDFK_DUAL_NC, SDFK_DUAL_NV, SDFK_PROJECT_GO);
#undef SDFK_PROJECT_GO
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sdfk_project_points_device(sdfk_program* p, const float* d_co, int64_t n, int64_t row_stride, float level,
                                          float tol, int max_iter, float relax, float* d_q, int64_t q_stride,
                                          float* d_value, float* d_grad, int64_t grad_stride, float* d_start,
                                          int32_t* d_info, void* stream) {
    return project_points(p, d_co, n, row_stride, level, tol, max_iter, relax, d_q, q_stride, d_value, d_grad, grad_stride,
                          d_start, d_info, nullptr, stream);
}

extern "C" int64_t sdfk_project_workgroups(int64_t n) { return n <= 0 ? 0 : (n + SDFK_BLOCK - 1) / SDFK_BLOCK; }

extern "C" int sdfk_project_points_counted_device(sdfk_program* p, const float* d_co, int64_t n, int64_t row_stride,
                                                  float level, float tol, int max_iter, float relax, float* d_q,
                                                  int64_t q_stride, float* d_value, float* d_grad, int64_t grad_stride,
                                                  float* d_start, int32_t* d_info, uint32_t* d_wg_trips, void* stream) {
    if (!d_wg_trips) return fail(-1, "sdfk_project_points_counted_device: null counter pointer");
    return project_points(p, d_co, n, row_stride, level, tol, max_iter, relax, d_q, q_stride, d_value, d_grad, grad_stride,
                          d_start, d_info, d_wg_trips, stream);
}
