// sdfk_adjoint.inc — reverse-mode derivatives of a program (included at the end of sdfk.hip, after sdfk_dual.inc).
//
//   * sdfk_vjp_kernel<NC, NV> : one pass of the dual kernel's register machine with a restore tape, then a reverse sweep
//     that back-propagates a per-point cotangent c_i and reduces P̄_j = Σ_i c_i ∂f_i/∂P_j over the points on the device.
//     Same program words, P and tables as sdfk_jvp_kernel; one point per lane, every instruction evaluated. The register
//     files (values and adjoints) are plain per-component float arrays, as in sdfk_dual.inc: VGPRs in the small
//     instantiation (2 / 3), scratch in the full one (16 / 8).
//   * Forward sweep: the sdfk_device.h function of each opcode (the interpreter's dispatch), so the value is the dual
//     kernel's value channel bit for bit. Before an instruction overwrites register a, the old contents of a are pushed on
//     a per-lane tape: 3 floats for a coordinate register, 1 for a value register. The tape is a private array of
//     SDFK_VJP_TAPE floats (scratch; the index is wave-uniform); the host refuses a program whose pushes exceed it.
//   * Reverse sweep, per instruction from the last: ā = adj[a]; adj[a] = 0; pop a (its inputs are then what they were
//     when it ran); adj[b] (and adj[c]) += the instruction's vector-Jacobian product, and the parameter part goes to P̄.
//     Zeroing before accumulating makes in-place instructions (a == b: the ROT2D halves) right.
//   * Local rules: the generic path derives each product from the opcode's DUAL rule (sdfk_dualdev.h) — the instruction's
//     own inputs and parameters are seeded as tangent channels, 4 at a time, through a local Q table with ns = NPARAMS,
//     and the resulting columns are dotted with ā. Every seed index is a compile-time constant, so Q folds away. The
//     affine ops and the cheapest combiners also have hand-written products (flags bit 0 turns them off; the tests
//     compare both paths).
//   * Reduction: a persistent grid (at most SDFK_VJP_GRID workgroups, fixed by n alone) walks the points with a
//     grid-stride loop. Per instruction and parameter, a wave sums its 64 lanes in fp32 (butterfly) and adds the sum in
//     float64 to its own row of an LDS accumulator (no atomics: one wave per row). At the end each workgroup folds its
//     waves' rows in order into one float64 row of a slab (SDFK_VJP_GRID x (n_params + 1)), and sdfk_vjp_sum_kernel adds
//     the slab's columns in workgroup order. Every sum has a fixed order: two calls give identical bits.
//   * SSE mode (mode 1): d_in is a target t; the cotangent is 2 (f_i - t_i), formed in registers, and the loss
//     Σ (f_i - t_i)² is accumulated in float64 in the extra column n_params.

#define SDFK_VJP_TAPE 256          // floats per lane of the restore tape (1 KiB of scratch)
#define SDFK_VJP_GRID 2048         // workgroups of the persistent grid at most
#define SDFK_VJP_WAVES (SDFK_BLOCK / 64)
#define SDFK_VJP_MAX_PARAMS 2047   // LDS: SDFK_VJP_WAVES rows of (n_params + 1) doubles <= 64 KiB

// 1 if the opcode has a dual rule (compile time; sdfk_dual_has_rule is the C-ABI twin)
static constexpr bool sdfk_dual_rule(int op) {
    switch (op) {
#define SDFK_DUAL_HAS(NAME, KIND, FN) case SDFK_OP_##NAME:
        SDFK_DUAL_TABLE(SDFK_DUAL_HAS)
#undef SDFK_DUAL_HAS
        return true;
        default:
            return false;
    }
}

// parameter count of an opcode (compile time)
static constexpr int sdfk_nparams(int op) {
    switch (op) {
#define SDFK_OP(NAME, KIND, NP, FUNC) \
    case SDFK_OP_##NAME:              \
        return NP;
#include "sdfk_ops.def"
#undef SDFK_OP
        default:
            return 0;
    }
}

// ---- the generic products: seeds 4 at a time through the dual rule -----------------------------------------------------
// Seed s of an instruction: its input components first (3 for a coordinate, 1 per value), then its parameters.
#define SDFK_VJP_SEEDQ(NI, NP, g)                                                   \
    float Q[4 * ((NP) > 0 ? (NP) : 1)];                                             \
    _Pragma("unroll") for (int k = 0; k < 4; ++k)                                   \
        _Pragma("unroll") for (int j = 0; j < (NP); ++j) Q[k * (NP) + j] = (4 * (g) + k == (NI) + j) ? 1.0f : 0.0f

// coordinate -> coordinate: gin[3] += ā·∂q/∂p, gp[j] = ā·∂q/∂P_j
template <int NP, typename F>
SDFK_DEV void vjp_generic_cc(F fn, V3 p, float ax, float ay, float az, float* gin, float* gp) {
    constexpr int S = 3 + NP, G = (S + 3) / 4;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        DC<4> c;
        c.x = p.x, c.y = p.y, c.z = p.z;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int s = 4 * g + k;
            c.dx[k] = s == 0 ? 1.0f : 0.0f, c.dy[k] = s == 1 ? 1.0f : 0.0f, c.dz[k] = s == 2 ? 1.0f : 0.0f;
        }
        SDFK_VJP_SEEDQ(3, NP, g);
        const DC<4> r = fn(c, Q, NP);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int s = 4 * g + k;
            const float v = ax * r.dx[k] + ay * r.dy[k] + az * r.dz[k];
            if (s < 3) gin[s] += v;
            else if (s < S) gp[s - 3] = v;
        }
    }
}
// coordinate -> value
template <int NP, typename F> SDFK_DEV void vjp_generic_vc(F fn, V3 p, float av, float* gin, float* gp) {
    constexpr int S = 3 + NP, G = (S + 3) / 4;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        DC<4> c;
        c.x = p.x, c.y = p.y, c.z = p.z;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int s = 4 * g + k;
            c.dx[k] = s == 0 ? 1.0f : 0.0f, c.dy[k] = s == 1 ? 1.0f : 0.0f, c.dz[k] = s == 2 ? 1.0f : 0.0f;
        }
        SDFK_VJP_SEEDQ(3, NP, g);
        const DS<4> r = fn(c, Q, NP);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int s = 4 * g + k;
            if (s < 3) gin[s] += av * r.d[k];
            else if (s < S) gp[s - 3] = av * r.d[k];
        }
    }
}
// value -> value
template <int NP, typename F> SDFK_DEV void vjp_generic_vv(F fn, float v, float av, float* gin, float* gp) {
    constexpr int S = 1 + NP, G = (S + 3) / 4;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        DS<4> a;
        a.v = v;
#pragma unroll
        for (int k = 0; k < 4; ++k) a.d[k] = 4 * g + k == 0 ? 1.0f : 0.0f;
        SDFK_VJP_SEEDQ(1, NP, g);
        const DS<4> r = fn(a, Q, NP);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int s = 4 * g + k;
            if (s < 1) gin[0] += av * r.d[k];
            else if (s < S) gp[s - 1] = av * r.d[k];
        }
    }
}
// (value, value) -> value: gin[0] for b, gin[1] for c (separate seeds, so b == c is right too)
template <int NP, typename F> SDFK_DEV void vjp_generic_vvv(F fn, float v1, float v2, float av, float* gin, float* gp) {
    constexpr int S = 2 + NP, G = (S + 3) / 4;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        DS<4> a, b;
        a.v = v1, b.v = v2;
#pragma unroll
        for (int k = 0; k < 4; ++k) a.d[k] = 4 * g + k == 0 ? 1.0f : 0.0f, b.d[k] = 4 * g + k == 1 ? 1.0f : 0.0f;
        SDFK_VJP_SEEDQ(2, NP, g);
        const DS<4> r = fn(a, b, Q, NP);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int s = 4 * g + k;
            if (s < 2) gin[s] += av * r.d[k];
            else if (s < S) gp[s - 2] = av * r.d[k];
        }
    }
}

// ---- hand-written products (same conventions as the dual rules; checked against the generic path by the tests) ---------
// returns false where the opcode has none
template <int OP>
SDFK_DEV bool vjp_hand_cc(V3 p, const float* __restrict__ P, float ax, float ay, float az, float* gin, float* gp) {
    if constexpr (OP == SDFK_OP_MOVC) {
        gin[0] += ax, gin[1] += ay, gin[2] += az;
        return true;
    } else if constexpr (OP == SDFK_OP_XLATE) {
        gin[0] += ax, gin[1] += ay, gin[2] += az;
        gp[0] = -ax, gp[1] = -ay, gp[2] = -az;
        return true;
    } else if constexpr (OP == SDFK_OP_XFORM || OP == SDFK_OP_LIN3) {       // q = M p (- c)
        gin[0] += P[0] * ax + P[3] * ay + P[6] * az;
        gin[1] += P[1] * ax + P[4] * ay + P[7] * az;
        gin[2] += P[2] * ax + P[5] * ay + P[8] * az;
        gp[0] = ax * p.x, gp[1] = ax * p.y, gp[2] = ax * p.z;
        gp[3] = ay * p.x, gp[4] = ay * p.y, gp[5] = ay * p.z;
        gp[6] = az * p.x, gp[7] = az * p.y, gp[8] = az * p.z;
        if constexpr (OP == SDFK_OP_XFORM) gp[9] = -ax, gp[10] = -ay, gp[11] = -az;
        return true;
    } else if constexpr (OP == SDFK_OP_CSCALE) {
        gin[0] += P[0] * ax, gin[1] += P[0] * ay, gin[2] += P[0] * az;
        gp[0] = ax * p.x + ay * p.y + az * p.z;
        return true;
    }
    return false;
}
template <int OP> SDFK_DEV bool vjp_hand_vvv(float v1, float v2, float av, float* gin) {
    if constexpr (OP == SDFK_OP_VMIN) {           // sdd_min: a's tangent at a tie
        if (v1 <= v2) gin[0] += av; else gin[1] += av;
        return true;
    } else if constexpr (OP == SDFK_OP_VMAX) {
        if (v1 >= v2) gin[0] += av; else gin[1] += av;
        return true;
    } else if constexpr (OP == SDFK_OP_VADD) {
        gin[0] += av, gin[1] += av;
        return true;
    }
    return false;
}

SDFK_DEV float vjp_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
SDFK_DEV double vjp_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <int NC, int NV>
__global__ __launch_bounds__(SDFK_BLOCK) void sdfk_vjp_kernel(const uint2* __restrict__ code, int n_instr,
                                                             const float* __restrict__ prm, int ns,
                                                             const float* __restrict__ tab, SrcArray src, long long n,
                                                             const float* __restrict__ d_in, int mode, int generic,
                                                             float* __restrict__ out_v, double* __restrict__ slab,
                                                             int result_reg) {
    extern __shared__ double vjp_acc[];                 // SDFK_VJP_WAVES rows of ns + 1 (the loss last)
    const int ns1 = ns + 1;
    const unsigned tid = sdfk_tx(), lane = tid & 63u, wave = tid >> 6;
    double* __restrict__ acc = vjp_acc + wave * ns1;
    for (int j = tid; j < SDFK_VJP_WAVES * ns1; j += SDFK_BLOCK) vjp_acc[j] = 0.0;
    __syncthreads();
    const long long step = (long long)sdfk_gx() * SDFK_BLOCK;
    for (long long base = (long long)sdfk_bx() * SDFK_BLOCK; base < n; base += step) {   // uniform over the workgroup
        const long long i = base + tid;
        const bool valid = i < n;
        const long long ii = valid ? i : n - 1;         // idle lanes run point n - 1 with a zero cotangent
        float Cx[NC], Cy[NC], Cz[NC], VV[NV];
        float ACx[NC], ACy[NC], ACz[NC], AV[NV];
        float tape[SDFK_VJP_TAPE];
        {
            V3 p[1];
            sdfk_load<1>(src, ii, 0, p);
#pragma unroll
            for (int r = 0; r < NC; ++r) Cx[r] = p[0].x, Cy[r] = p[0].y, Cz[r] = p[0].z, ACx[r] = ACy[r] = ACz[r] = 0.0f;
#pragma unroll
            for (int r = 0; r < NV; ++r) VV[r] = 0.0f, AV[r] = 0.0f;
        }
        // ---- forward sweep
        int t = 0;
        for (int pc = 0; pc < n_instr; ++pc) {
            const uint2 ins = code[pc];                 // wave-uniform: scalar loads
            const unsigned op = ins.x & 255u, a = (ins.x >> 8) & 255u, b = (ins.x >> 16) & 255u, c = ins.x >> 24;
            const float* __restrict__ P = prm + ins.y;
            switch (op) {
#define SDFK_VJP_FWD_C_C(F)                                             \
    {                                                                   \
        tape[t] = Cx[a], tape[t + 1] = Cy[a], tape[t + 2] = Cz[a];      \
        t += 3;                                                         \
        const V3 q = F(V3{Cx[b], Cy[b], Cz[b]}, P, tab, (int)c);        \
        Cx[a] = q.x, Cy[a] = q.y, Cz[a] = q.z;                          \
    }
#define SDFK_VJP_FWD_V_C(F)                                             \
    {                                                                   \
        tape[t++] = VV[a];                                              \
        VV[a] = F(V3{Cx[b], Cy[b], Cz[b]}, P, tab);                     \
    }
#define SDFK_VJP_FWD_V_V(F)                                             \
    {                                                                   \
        tape[t++] = VV[a];                                              \
        VV[a] = F(VV[b], P);                                            \
    }
#define SDFK_VJP_FWD_V_VV(F)                                            \
    {                                                                   \
        tape[t++] = VV[a];                                              \
        VV[a] = F(VV[b], VV[c], P);                                     \
    }
#define SDFK_OP(NAME, KIND, NP, FUNC)            \
    case SDFK_OP_##NAME:                         \
        if constexpr (sdfk_dual_rule(SDFK_OP_##NAME)) SDFK_VJP_FWD_##KIND(FUNC); \
        break;
#include "sdfk_ops.def"
#undef SDFK_OP
                default:                                // refused on the host (sdfk_program_vjp_check)
                    break;
            }
        }
        const float f = VV[result_reg];
        float cot = 0.0f;
        double loss = 0.0;
        if (valid) {
            if (out_v) out_v[i] = f;
            if (mode == 1) {
                const float tg = d_in[i];
                cot = 2.0f * (f - tg);
                const double d = (double)f - (double)tg;
                loss = d * d;
            } else {
                cot = d_in[i];
            }
        }
        AV[result_reg] = cot;
        // ---- reverse sweep
        for (int pc = n_instr - 1; pc >= 0; --pc) {
            const uint2 ins = code[pc];
            const unsigned op = ins.x & 255u, a = (ins.x >> 8) & 255u, b = (ins.x >> 16) & 255u, c = ins.x >> 24;
            const float* __restrict__ P = prm + ins.y;
            switch (op) {
// parameter adjoints: one wave sum per parameter of the instruction (ins.y is wave-uniform), added in float64 to the
// wave's own accumulator row
#define SDFK_VJP_REDUCE(NP)                                                                                  \
    _Pragma("unroll") for (int j = 0; j < (NP); ++j) {                                                       \
        const float s_ = vjp_wave_sum(valid ? gp[j] : 0.0f);                                                 \
        if (lane == 0) acc[ins.y + j] += (double)s_;                                                         \
    }
#define SDFK_VJP_REV_C_C(OP, FN)                                                                             \
    {                                                                                                        \
        constexpr int NP = sdfk_nparams(OP);                                                                 \
        float gp[NP > 0 ? NP : 1];                                                                           \
        const float ax = ACx[a], ay = ACy[a], az = ACz[a];                                                   \
        ACx[a] = ACy[a] = ACz[a] = 0.0f;                                                                     \
        t -= 3;                                                                                              \
        Cx[a] = tape[t], Cy[a] = tape[t + 1], Cz[a] = tape[t + 2];                                           \
        const V3 p = {Cx[b], Cy[b], Cz[b]};                                                                  \
        float gin[3] = {0.0f, 0.0f, 0.0f};                                                                   \
        if (generic || !vjp_hand_cc<OP>(p, P, ax, ay, az, gin, gp))                                          \
            vjp_generic_cc<NP>([&](const DC<4>& x, const float* Q, int q_ns) { return FN<4>(x, P, Q, q_ns, tab, (int)c); }, \
                               p, ax, ay, az, gin, gp);                                                      \
        ACx[b] += gin[0], ACy[b] += gin[1], ACz[b] += gin[2];                                                \
        SDFK_VJP_REDUCE(NP);                                                                                 \
    }
#define SDFK_VJP_REV_V_C(OP, FN)                                                                             \
    {                                                                                                        \
        constexpr int NP = sdfk_nparams(OP);                                                                 \
        float gp[NP > 0 ? NP : 1];                                                                           \
        const float av = AV[a];                                                                              \
        AV[a] = 0.0f;                                                                                        \
        VV[a] = tape[--t];                                                                                   \
        float gin[3] = {0.0f, 0.0f, 0.0f};                                                                   \
        vjp_generic_vc<NP>([&](const DC<4>& x, const float* Q, int q_ns) { return FN<4>(x, P, Q, q_ns, tab); }, \
                           V3{Cx[b], Cy[b], Cz[b]}, av, gin, gp);                                            \
        ACx[b] += gin[0], ACy[b] += gin[1], ACz[b] += gin[2];                                                \
        SDFK_VJP_REDUCE(NP);                                                                                 \
    }
#define SDFK_VJP_REV_V_V(OP, FN)                                                                             \
    {                                                                                                        \
        constexpr int NP = sdfk_nparams(OP);                                                                 \
        float gp[NP > 0 ? NP : 1];                                                                           \
        const float av = AV[a];                                                                              \
        AV[a] = 0.0f;                                                                                        \
        VV[a] = tape[--t];                                                                                   \
        float gin[1] = {0.0f};                                                                               \
        vjp_generic_vv<NP>([&](const DS<4>& x, const float* Q, int q_ns) { return FN<4>(x, P, Q, q_ns); },   \
                           VV[b], av, gin, gp);                                                              \
        AV[b] += gin[0];                                                                                     \
        SDFK_VJP_REDUCE(NP);                                                                                 \
    }
#define SDFK_VJP_REV_V_VV(OP, FN)                                                                            \
    {                                                                                                        \
        constexpr int NP = sdfk_nparams(OP);                                                                 \
        float gp[NP > 0 ? NP : 1];                                                                           \
        const float av = AV[a];                                                                              \
        AV[a] = 0.0f;                                                                                        \
        VV[a] = tape[--t];                                                                                   \
        float gin[2] = {0.0f, 0.0f};                                                                         \
        if (generic || !vjp_hand_vvv<OP>(VV[b], VV[c], av, gin))                                             \
            vjp_generic_vvv<NP>([&](const DS<4>& x, const DS<4>& y, const float* Q, int q_ns) {              \
                return FN<4>(x, y, P, Q, q_ns); }, VV[b], VV[c], av, gin, gp);                               \
        AV[b] += gin[0];                                                                                     \
        AV[c] += gin[1];                                                                                     \
        SDFK_VJP_REDUCE(NP);                                                                                 \
    }
#define SDFK_VJP_CASE(NAME, KIND, FN)               \
    case SDFK_OP_##NAME:                            \
        SDFK_VJP_REV_##KIND(SDFK_OP_##NAME, FN);    \
        break;
                SDFK_DUAL_TABLE(SDFK_VJP_CASE)
#undef SDFK_VJP_CASE
                default:
                    break;
            }
        }
        if (mode == 1) {
            const double s = vjp_wave_sum(loss);
            if (lane == 0) acc[ns] += s;
        }
    }
    __syncthreads();
    double* __restrict__ row = slab + (long long)sdfk_bx() * ns1;
    for (int j = tid; j < ns1; j += SDFK_BLOCK) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < SDFK_VJP_WAVES; ++w) s += vjp_acc[w * ns1 + j];
        row[j] = s;
    }
}

// column sums of the slab in workgroup order
__global__ __launch_bounds__(SDFK_BLOCK) void sdfk_vjp_sum_kernel(const double* __restrict__ slab, int rows, int ns1,
                                                                 double* __restrict__ out) {
    const int j = (int)(sdfk_bx() * SDFK_BLOCK + sdfk_tx());
    if (j >= ns1) return;
    double s = 0.0;
    for (int r = 0; r < rows; ++r) s += slab[(long long)r * ns1 + j];
    out[j] = s;
}

// ---- host side ----------------------------------------------------------------------------------
// floats of the restore tape a program pushes per point
static long long vjp_tape_floats(const sdfk_program* p) {
    long long t = 0;
    for (size_t i = 0; i < p->code.size() / 2; ++i) t += g_ops[p->code[2 * i] & 255u].kind == SDFK_KIND_C_C ? 3 : 1;
    return t;
}

extern "C" int sdfk_program_vjp_check(sdfk_program* p, int* first_bad_op, int64_t* tape_floats) {
    if (!p) return fail(-1, "null program");
    const long long tape = vjp_tape_floats(p);
    if (tape_floats) *tape_floats = tape;
    const int rc = sdfk_program_jvp_check(p, first_bad_op);
    if (rc) return rc;
    if (tape > SDFK_VJP_TAPE) {
        g_err = "program too large for the adjoint kernel: its restore tape takes " + std::to_string(tape) +
                " floats per point, " + std::to_string(SDFK_VJP_TAPE) + " at most";
        return 3;
    }
    if (p->params.size() > SDFK_VJP_MAX_PARAMS) {
        g_err = "program too large for the adjoint kernel: " + std::to_string(p->params.size()) + " parameters, " +
                std::to_string(SDFK_VJP_MAX_PARAMS) + " at most";
        return 4;
    }
    return 0;
}

extern "C" int sdfk_vjp_limits(int* tape_floats, int* max_params) {
    if (tape_floats) *tape_floats = SDFK_VJP_TAPE;
    if (max_params) *max_params = SDFK_VJP_MAX_PARAMS;
    return 0;
}

extern "C" int sdfk_eval_vjp_device(sdfk_program* p, const float* d_co, int64_t n, int64_t row_stride, const float* d_in,
                                    int mode, int flags, float* d_out_value, double* h_pbar, double* h_loss, void* stream) {
    if (!p) return fail(-1, "null program");
    if (!h_pbar && p->params.size()) return fail(-1, "sdfk_eval_vjp_device: null parameter-adjoint buffer");
    if (mode != 0 && mode != 1) return fail(-1, "sdfk_eval_vjp_device: mode is 0 (cotangent) or 1 (sum of squares)");
    if (n < 0 || row_stride < n) return fail(-1, "sdfk_eval_vjp_device: row stride smaller than the point count");
    if (n > 0 && (!d_co || !d_in)) return fail(-1, "sdfk_eval_vjp_device: null device pointer");
    const int chk = sdfk_program_vjp_check(p, nullptr, nullptr);
    if (chk) return fail(chk < 0 ? chk : -3, "sdfk_eval_vjp_device: " + g_err);
    const int ns = (int)p->params.size(), ns1 = ns + 1;
    if (n == 0) {
        for (int j = 0; j < ns; ++j) h_pbar[j] = 0.0;
        if (h_loss) *h_loss = 0.0;
        return 0;
    }
    LaunchCtx x;
    const int rc = launch_ctx(p, stream, &x);
    if (rc) return rc;
    hipStream_t s = x.stream;
    const long long need = (n + SDFK_BLOCK - 1) / SDFK_BLOCK;
    const unsigned blocks = (unsigned)std::min<long long>(need, SDFK_VJP_GRID);      // a function of n only
    double* d_ws = nullptr;
    HIPCHK(hipMalloc(&d_ws, ((size_t)blocks + 1) * ns1 * sizeof(double)));
    double* d_sum = d_ws + (size_t)blocks * ns1;
    SrcArray src = {d_co, (long long)row_stride};
    const size_t lds = (size_t)SDFK_VJP_WAVES * ns1 * sizeof(double);
    const int generic = flags & 1;
#define SDFK_VJP_GO(NC, NV) hipLaunchKernelGGL((sdfk_vjp_kernel<NC, NV>), dim3(blocks), dim3(SDFK_BLOCK), lds, s, x.d->d_code, x.n_instr, \
                                               x.prm, ns, x.tab, src, (long long)n, d_in, mode, generic, d_out_value, d_ws, x.result_reg)
    SDFK_REGFILE(p, SDFK_DUAL_NC, SDFK_DUAL_NV, SDFK_VJP_GO);
#undef SDFK_VJP_GO
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(sdfk_vjp_sum_kernel, dim3((ns1 + SDFK_BLOCK - 1) / SDFK_BLOCK), dim3(SDFK_BLOCK), 0, s, d_ws,
                           (int)blocks, ns1, d_sum);
        e = hipGetLastError();
    }
    std::vector<double> host(ns1);
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), d_sum, ns1 * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d_ws);
    HIPCHK(e);
    for (int j = 0; j < ns; ++j) h_pbar[j] = host[j];
    if (h_loss) *h_loss = mode == 1 ? host[ns] : 0.0;
    return 0;
}
