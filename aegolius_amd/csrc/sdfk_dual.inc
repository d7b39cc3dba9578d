// sdfk_dual.inc — forward-mode derivatives of a program (included at the end of sdfk.hip; rules in sdfk_dualdev.h).
//
//   * sdfk_jvp_kernel<K, NC, NV, SRC> : the interpreter's register machine on dual numbers. Same program words, same P,
//     plus a K x n_params table dP of parameter tangents. A coordinate register is 3 (1 + K) floats, a value register
//     1 + K. One point per lane (VEC = 1), every instruction evaluated (no culling, no hiprtc specialisation).
//     Register files: plain per-component float arrays (below). The small instantiation (NC = 2, NV = 3, the
//     interpreter's SDFK_NC_SMALL / SDFK_NV_SMALL) is held in VGPRs; the full one (NC = 16, NV = 8) is the same code and
//     lives in scratch. It has twice the
//     interpreter's coordinate registers because the shortcut-free lowering the derivatives need never aliases an
//     identity transform: a left-deep chain of n combinations holds n + 1 coordinate registers (BASELINE cfg 2: 10).
//   * sdfk_value_jvp_kernel : one V_V rule elementwise on (value, tangent) pairs (post-processing maps, chain rule).
// Traffic of sdfk_jvp_kernel: 12 B of coordinates in, 4 (1 + K) B out per point.
#include "sdfk_dualdev.h"

#define SDFK_DUAL_NC 16
#define SDFK_DUAL_NV 8

// Register files as plain per-component float arrays indexed by the (wave-uniform) register number — the interpreter's
// SPLIT layout (sdfk.hip sdfk_interp_kernel): small arrays of scalars are promoted to VGPRs, whereas arrays of the
// DC<K> / DS<K> structs (or unrolled selects over them) end up as an indexed array in scratch. Tangent channel k of
// register r is element r * K + k of its component's array.
#define SDFK_CF_GET(F, r, out)                                                                     \
    do {                                                                                           \
        const unsigned r_ = (r);                                                                   \
        (out).x = F##x[r_], (out).y = F##y[r_], (out).z = F##z[r_];                                \
        SDFK_KLOOP(out).dx[k] = F##tx[r_ * K + k], (out).dy[k] = F##ty[r_ * K + k], (out).dz[k] = F##tz[r_ * K + k]; \
    } while (0)
#define SDFK_CF_SET(F, r, val)                                                                     \
    do {                                                                                           \
        const unsigned r_ = (r);                                                                   \
        const DC<K> v_ = (val);                                                                    \
        F##x[r_] = v_.x, F##y[r_] = v_.y, F##z[r_] = v_.z;                                         \
        SDFK_KLOOP F##tx[r_ * K + k] = v_.dx[k], F##ty[r_ * K + k] = v_.dy[k], F##tz[r_ * K + k] = v_.dz[k]; \
    } while (0)
#define SDFK_VF_GET(r, out)                                                                        \
    do {                                                                                           \
        const unsigned r_ = (r);                                                                   \
        (out).v = VV[r_];                                                                          \
        SDFK_KLOOP(out).d[k] = VT[r_ * K + k];                                                     \
    } while (0)
#define SDFK_VF_SET(r, val)                                                                        \
    do {                                                                                           \
        const unsigned r_ = (r);                                                                   \
        const DS<K> v_ = (val);                                                                    \
        VV[r_] = v_.v;                                                                             \
        SDFK_KLOOP VT[r_ * K + k] = v_.d[k];                                                       \
    } while (0)

template <int K, int NC, int NV, typename SRC>
__global__ __launch_bounds__(SDFK_BLOCK) void sdfk_jvp_kernel(const uint2* __restrict__ code, int n_instr,
                                                             const float* __restrict__ prm, const float* __restrict__ dprm,
                                                             int ns, const float* __restrict__ tab, SRC src, long long n,
                                                             int seed_points, float* __restrict__ out_v,
                                                             float* __restrict__ out_t, long long tstride, int result_reg) {
    const long long block_base = (long long)sdfk_bx() * SDFK_BLOCK;
    const unsigned lane = sdfk_tx();
    const long long i = block_base + lane;
    if (i >= n) return;
    float Cx[NC], Cy[NC], Cz[NC], Ctx[NC * K], Cty[NC * K], Ctz[NC * K];
    float VV[NV], VT[NV * K];
    {
        V3 p[1];
        sdfk_load<1>(src, block_base, lane, p);
#pragma unroll
        for (int r = 0; r < NC; ++r) {
            Cx[r] = p[0].x, Cy[r] = p[0].y, Cz[r] = p[0].z;
            SDFK_KLOOP {
                Ctx[r * K + k] = (seed_points && k == 0) ? 1.0f : 0.0f;
                Cty[r * K + k] = (seed_points && k == 1) ? 1.0f : 0.0f;
                Ctz[r * K + k] = (seed_points && k == 2) ? 1.0f : 0.0f;
            }
        }
#pragma unroll
        for (int r = 0; r < NV; ++r) {
            VV[r] = 0.0f;
            SDFK_KLOOP VT[r * K + k] = 0.0f;
        }
    }
    for (int pc = 0; pc < n_instr; ++pc) {
        const uint2 ins = code[pc];                     // wave-uniform: scalar loads
        const unsigned op = ins.x & 255u, a = (ins.x >> 8) & 255u, b = (ins.x >> 16) & 255u, c = ins.x >> 24;
        const float* __restrict__ P = prm + ins.y;
        const float* __restrict__ Q = dprm + ins.y;
        switch (op) {
#define SDFK_DUAL_EXEC_C_C(FN)                              \
    {                                                       \
        DC<K> in;                                           \
        SDFK_CF_GET(C, b, in);                              \
        SDFK_CF_SET(C, a, FN<K>(in, P, Q, ns, tab, (int)c)); \
    }
#define SDFK_DUAL_EXEC_V_C(FN)                        \
    {                                                 \
        DC<K> in;                                     \
        SDFK_CF_GET(C, b, in);                        \
        SDFK_VF_SET(a, FN<K>(in, P, Q, ns, tab));     \
    }
#define SDFK_DUAL_EXEC_V_V(FN)                        \
    {                                                 \
        DS<K> in;                                     \
        SDFK_VF_GET(b, in);                           \
        SDFK_VF_SET(a, FN<K>(in, P, Q, ns));          \
    }
#define SDFK_DUAL_EXEC_V_VV(FN)                       \
    {                                                 \
        DS<K> in1, in2;                               \
        SDFK_VF_GET(b, in1);                          \
        SDFK_VF_GET(c, in2);                          \
        SDFK_VF_SET(a, FN<K>(in1, in2, P, Q, ns));    \
    }
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
    out_v[i] = r.v;
    SDFK_KLOOP out_t[k * tstride + i] = r.d[k];
}

struct SdfkPBlock {
    float p[8];
};

__global__ __launch_bounds__(SDFK_BLOCK) void sdfk_value_jvp_kernel(int op, SdfkPBlock blk, const float* __restrict__ v,
                                                                   const float* __restrict__ t, long long n,
                                                                   float* __restrict__ ov, float* __restrict__ ot) {
    const long long i = (long long)sdfk_bx() * SDFK_BLOCK + sdfk_tx();
    if (i >= n) return;
    float P[8], Z[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) P[j] = blk.p[j], Z[j] = 0.0f;
    DS<1> a;
    a.v = v[i];
    a.d[0] = t[i];
    DS<1> r = a;
    switch (op) {
#define SDFK_VJ_CASE_C_C(NAME, FN)
#define SDFK_VJ_CASE_V_C(NAME, FN)
#define SDFK_VJ_CASE_V_VV(NAME, FN)
#define SDFK_VJ_CASE_V_V(NAME, FN) \
    case SDFK_OP_##NAME:           \
        r = FN<1>(a, P, Z, 0);     \
        break;
#define SDFK_VJ_CASE(NAME, KIND, FN) SDFK_VJ_CASE_##KIND(NAME, FN)
        SDFK_DUAL_TABLE(SDFK_VJ_CASE)
#undef SDFK_VJ_CASE
        default:
            break;
    }
    ov[i] = r.v;
    ot[i] = r.d[0];
}

// ---- host side ----------------------------------------------------------------------------------
extern "C" int sdfk_dual_has_rule(int op) {
    switch (op) {
#define SDFK_DUAL_HAS(NAME, KIND, FN) case SDFK_OP_##NAME:
        SDFK_DUAL_TABLE(SDFK_DUAL_HAS)
#undef SDFK_DUAL_HAS
        return 1;
        default:
            return 0;
    }
}

// coordinate / value registers the program touches (the result register included)
static void dual_regs(const sdfk_program* p, int* nc, int* nv) {
    unsigned mc = 0, mv = (unsigned)p->result_reg;
    for (size_t i = 0; i < p->code.size() / 2; ++i) {
        const uint32_t w = p->code[2 * i];
        const unsigned op = w & 255u, a = (w >> 8) & 255u, b = (w >> 16) & 255u, c = w >> 24;
        switch (g_ops[op].kind) {
            case SDFK_KIND_C_C: mc = std::max(mc, std::max(a, b)); break;
            case SDFK_KIND_V_C: mc = std::max(mc, b); mv = std::max(mv, a); break;
            case SDFK_KIND_V_V: mv = std::max(mv, std::max(a, b)); break;
            default: mv = std::max(mv, std::max(a, std::max(b, c))); break;
        }
    }
    *nc = (int)mc + 1;
    *nv = (int)mv + 1;
}

extern "C" int sdfk_program_jvp_check(sdfk_program* p, int* first_bad_op) {
    if (!p) return fail(-1, "null program");
    if (first_bad_op) *first_bad_op = -1;
    const size_t n_instr = p->code.size() / 2;
    for (size_t i = 0; i < n_instr; ++i) {
        const unsigned op = p->code[2 * i] & 255u;
        if (!sdfk_dual_has_rule((int)op)) {
            if (first_bad_op) *first_bad_op = (int)i;
            char buf[160];
            snprintf(buf, sizeof buf, "instruction %zu (%s): no dual rule", i, g_ops[op].name);
            g_err = buf;
            return 1;
        }
    }
    int nc = 0, nv = 0;
    dual_regs(p, &nc, &nv);
    if (nc > SDFK_DUAL_NC || nv > SDFK_DUAL_NV) {
        g_err = "program too large for the dual kernel";
        return 2;
    }
    return 0;
}

template <int NC, int NV>
static void launch_jvp(int k, unsigned blocks, hipStream_t s, const uint2* code, int n_instr, const float* prm,
                       const float* dprm, int ns, const float* tab, SrcArray src, long long n, int seed, float* ov,
                       float* ot, long long tstride, int res) {
    switch (k) {
#define SDFK_JVP_LAUNCH(KK)                                                                                              \
    case KK:                                                                                                             \
        hipLaunchKernelGGL((sdfk_jvp_kernel<KK, NC, NV, SrcArray>), dim3(blocks), dim3(SDFK_BLOCK), 0, s, code, n_instr, \
                           prm, dprm, ns, tab, src, n, seed, ov, ot, tstride, res);                                      \
        break;
        SDFK_JVP_LAUNCH(1) SDFK_JVP_LAUNCH(2) SDFK_JVP_LAUNCH(3) SDFK_JVP_LAUNCH(4)
#undef SDFK_JVP_LAUNCH
        default:
            break;
    }
}

extern "C" int sdfk_eval_jvp_device(sdfk_program* p, const float* d_co, int64_t n, int64_t row_stride,
                                    const float* d_dparams, int k, int seed_points, float* d_value, float* d_tangent,
                                    int64_t tangent_stride, void* stream) {
    if (!p) return fail(-1, "null program");
    if (!d_co || !d_dparams || !d_value || !d_tangent) return fail(-1, "sdfk_eval_jvp_device: null device pointer");
    if (k < 1 || k > 4) return fail(-1, "sdfk_eval_jvp_device: 1 to 4 tangent channels per launch");
    if (seed_points && k != 3) return fail(-1, "sdfk_eval_jvp_device: point mode takes exactly 3 channels");
    if (n < 0 || row_stride < n || tangent_stride < n)
        return fail(-1, "sdfk_eval_jvp_device: row or tangent stride smaller than the point count");
    int bad = -1;
    const int chk = sdfk_program_jvp_check(p, &bad);
    if (chk) return fail(chk < 0 ? chk : -3, "sdfk_eval_jvp_device: " + g_err);
    if (n == 0) return 0;
    LaunchCtx x;
    const int rc = launch_ctx(p, stream, &x);
    if (rc) return rc;
    const unsigned blocks = (unsigned)((n + SDFK_BLOCK - 1) / SDFK_BLOCK);
    SrcArray src = {d_co, (long long)row_stride};
    const int ns = (int)p->params.size();
#define SDFK_JVP_GO(NC, NV) launch_jvp<NC, NV>(k, blocks, x.stream, x.d->d_code, x.n_instr, x.prm, d_dparams, ns, x.tab, src, n, \
                                               seed_points, d_value, d_tangent, tangent_stride, x.result_reg)
    SDFK_REGFILE(p, SDFK_DUAL_NC, SDFK_DUAL_NV, SDFK_JVP_GO);
#undef SDFK_JVP_GO
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sdfk_value_jvp_device(int op, const float* P, const float* d_v, const float* d_t, int64_t n,
                                     float* d_out_v, float* d_out_t, void* stream) {
    if (op < 0 || op >= SDFK_OP_COUNT || g_ops[op].kind != SDFK_KIND_V_V || !sdfk_dual_has_rule(op))
        return fail(-1, "sdfk_value_jvp_device: not a value operation with a dual rule");
    if (g_ops[op].nparams > 8 || (g_ops[op].nparams > 0 && !P)) return fail(-1, "sdfk_value_jvp_device: bad parameters");
    if (!d_v || !d_t || !d_out_v || !d_out_t) return fail(-1, "sdfk_value_jvp_device: null device pointer");
    if (n < 0) return fail(-1, "negative point count");
    if (n == 0) return 0;
    SdfkPBlock blk = {};
    for (int j = 0; j < g_ops[op].nparams; ++j) blk.p[j] = P[j];
    const unsigned blocks = (unsigned)((n + SDFK_BLOCK - 1) / SDFK_BLOCK);
    hipLaunchKernelGGL(sdfk_value_jvp_kernel, dim3(blocks), dim3(SDFK_BLOCK), 0, (hipStream_t)stream, op, blk, d_v, d_t,
                       (long long)n, d_out_v, d_out_t);
    HIPCHK(hipGetLastError());
    return 0;
}
