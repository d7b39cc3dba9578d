// sdfk_interpfield.h — the interpreter's register machine as a __device__ evaluation of ONE point: the opcode switch
// instantiated from sdfk_ops.def once more, as the dual and adjoint kernels do. The field object of the interpreter
// kernels that evaluate point by point inside a loop of their own: the marches (sdfk_rays.inc) and the occupancy sample
// pass (sdfk_occupancy.inc). Included inside sdfk.hip, after the device functions of the opcodes.
#ifndef SDFK_INTERPFIELD_H
#define SDFK_INTERPFIELD_H


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

#endif  // SDFK_INTERPFIELD_H
