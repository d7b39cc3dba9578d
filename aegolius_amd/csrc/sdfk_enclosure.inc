// sdfk_enclosure.inc — interval enclosures of a program over boxes (included at the end of sdfk.hip; rules in
// sdfk_boxdev.h; Python: aegolius_amd/enclosure.py).
//
//   * sdfk_enclose_kernel<NC, NV>        : the interpreter's register machine on boxes. Same program words, same P, plus
//     one float per instruction (Lipschitz factors, see sdfk_boxdev.h). One box per lane, every instruction evaluated (no
//     culling, no hiprtc specialisation). Register files with the limits of sdfk_dual.inc: the small instantiation
//     (SDFK_NC_SMALL / SDFK_NV_SMALL) in VGPRs, the full one (SDFK_DUAL_NC / SDFK_DUAL_NV) in scratch (see sdfk_box_run).
//     Traffic: 24 B of box ends in, 8 B out.
//   * sdfk_enclose_octree_kernel<NC, NV> : one refinement step of an octree (quadtree for a 2-D domain) over box keys:
//     box of the key in float64, rounded outward to fp32, enclosed, classified against a level; the children of the mixed
//     boxes are appended to a list (wave-level prefix count, one atomic per wave, never past the capacity).
// Key: level << 57 | ix << 38 | iy << 19 | iz, coordinates 0 .. 2^level - 1 (level <= 19).
#include "sdfk_boxdev.h"

#define SDFK_BOX_KEY_BITS 19
#define SDFK_BOX_KEY_MASK 0x7ffffull

// the program on one box -> enclosure of the result register; NaN never leaves (an end that is NaN becomes its infinity)
template <int NC, int NV>
SDFK_DEV BV sdfk_box_run(const uint2* __restrict__ code, int n_instr, const float* __restrict__ prm,
                         const float* __restrict__ fac, const float* __restrict__ tab, int result_reg, const BC& start) {
    // The small coordinate file is seven plain float arrays, which the compiler keeps in VGPRs; the full one is an array
    // of structs and lives in scratch, as in the interpreter kernel (sdfk.hip): as plain arrays it is promoted to VGPRs
    // too — 256 of them and 5 AGPRs, with spills, one wave per SIMD.
    constexpr bool SPLIT = NC <= SDFK_NC_SMALL;
    float Bcx[SPLIT ? NC : 1], Bcy[SPLIT ? NC : 1], Bcz[SPLIT ? NC : 1], Bex[SPLIT ? NC : 1], Bey[SPLIT ? NC : 1], Bez[SPLIT ? NC : 1],
        Br[SPLIT ? NC : 1];
    BC BS[SPLIT ? 1 : NC];
    float Vlo[NV], Vhi[NV];
#define SDFK_BC_GET(reg, out)                                                                                    \
    do {                                                                                                         \
        const unsigned r_ = (reg);                                                                               \
        if constexpr (SPLIT) {                                                                                   \
            (out).cx = Bcx[SPLIT ? r_ : 0], (out).cy = Bcy[SPLIT ? r_ : 0], (out).cz = Bcz[SPLIT ? r_ : 0];      \
            (out).ex = Bex[SPLIT ? r_ : 0], (out).ey = Bey[SPLIT ? r_ : 0], (out).ez = Bez[SPLIT ? r_ : 0];      \
            (out).r = Br[SPLIT ? r_ : 0];                                                                        \
        } else                                                                                                   \
            (out) = BS[SPLIT ? 0 : r_];                                                                          \
    } while (0)
#define SDFK_BC_SET(reg, val)                                                                                    \
    do {                                                                                                         \
        const unsigned r_ = (reg);                                                                               \
        const BC v_ = (val);                                                                                     \
        if constexpr (SPLIT) {                                                                                   \
            Bcx[SPLIT ? r_ : 0] = v_.cx, Bcy[SPLIT ? r_ : 0] = v_.cy, Bcz[SPLIT ? r_ : 0] = v_.cz;               \
            Bex[SPLIT ? r_ : 0] = v_.ex, Bey[SPLIT ? r_ : 0] = v_.ey, Bez[SPLIT ? r_ : 0] = v_.ez;               \
            Br[SPLIT ? r_ : 0] = v_.r;                                                                           \
        } else                                                                                                   \
            BS[SPLIT ? 0 : r_] = v_;                                                                             \
    } while (0)
#pragma unroll
    for (int r = 0; r < NC; ++r) SDFK_BC_SET(r, start);
#pragma unroll
    for (int r = 0; r < NV; ++r) Vlo[r] = 0.0f, Vhi[r] = 0.0f;
#define SDFK_BV_SET(reg, val)              \
    do {                                  \
        const unsigned r_ = (reg);         \
        const BV v_ = (val);              \
        Vlo[r_] = v_.lo, Vhi[r_] = v_.hi; \
    } while (0)
    for (int pc = 0; pc < n_instr; ++pc) {
        const uint2 ins = code[pc];                     // wave-uniform: scalar loads
        const unsigned op = ins.x & 255u, a = (ins.x >> 8) & 255u, b = (ins.x >> 16) & 255u, c = ins.x >> 24;
        const float* __restrict__ P = prm + ins.y;
        const float F = fac[pc];
        switch (op) {
#define SDFK_BOX_EXEC_C_C(FN)                            \
    {                                                    \
        BC in;                                           \
        SDFK_BC_GET(b, in);                              \
        SDFK_BC_SET(a, FN(in, P, tab, (int)c, F));       \
    }
#define SDFK_BOX_EXEC_V_P(FN)                                    \
    {                                                            \
        BC in;                                                   \
        SDFK_BC_GET(b, in);                                      \
        SDFK_BV_SET(a, box_prim(FN(bc_c(in), P, tab), in, F));   \
    }
#define SDFK_BOX_EXEC_V_S(FN)                                    \
    {                                                            \
        BC in;                                                   \
        SDFK_BC_GET(b, in);                                      \
        SDFK_BV_SET(a, box_sign(0.0f, in, F));                   \
    }
#define SDFK_BOX_EXEC_V_V(FN)                 \
    {                                         \
        const BV in = {Vlo[b], Vhi[b]};       \
        SDFK_BV_SET(a, FN(in, P));            \
    }
#define SDFK_BOX_EXEC_V_VV(FN)                                    \
    {                                                             \
        const BV in1 = {Vlo[b], Vhi[b]}, in2 = {Vlo[c], Vhi[c]};  \
        SDFK_BV_SET(a, FN(in1, in2, P));                          \
    }
#define SDFK_BOX_CASE(NAME, KIND, FN) \
    case SDFK_OP_##NAME:              \
        SDFK_BOX_EXEC_##KIND(FN);     \
        break;
            SDFK_BOX_TABLE(SDFK_BOX_CASE)
#undef SDFK_BOX_CASE
            default:                                    // refused on the host (sdfk_program_box_check)
                break;
        }
    }
    BV r = {Vlo[result_reg], Vhi[result_reg]};
    if (bx_isnan(r.lo)) r.lo = -bx_inf();
    if (bx_isnan(r.hi)) r.hi = bx_inf();
    return r;
}

// coordinate register of the box [lo, hi] (fp32 ends): centre, extents to the farther end, half diagonal. Their own
// roundings (an ulp of the extent) are inside the padding of whichever rule reads them first.
SDFK_DEV BC sdfk_box_start(float lx, float ly, float lz, float hx, float hy, float hz) {
    BC b;
    b.cx = 0.5f * lx + 0.5f * hx, b.cy = 0.5f * ly + 0.5f * hy, b.cz = 0.5f * lz + 0.5f * hz;
    b.ex = sd_max(hx - b.cx, b.cx - lx), b.ey = sd_max(hy - b.cy, b.cy - ly), b.ez = sd_max(hz - b.cz, b.cz - lz);
    b.r = sd_len3(b.ex, b.ey, b.ez);
    return b;
}

template <int NC, int NV>
__global__ __launch_bounds__(SDFK_BLOCK) void sdfk_enclose_kernel(const uint2* __restrict__ code, int n_instr,
                                                                 const float* __restrict__ prm, const float* __restrict__ fac,
                                                                 const float* __restrict__ tab, const float* __restrict__ lo,
                                                                 const float* __restrict__ hi, long long stride, long long n,
                                                                 float* __restrict__ out_lo, float* __restrict__ out_hi,
                                                                 int result_reg) {
    const long long i = (long long)sdfk_bx() * SDFK_BLOCK + sdfk_tx();
    if (i >= n) return;
    const BC start = sdfk_box_start(lo[i], lo[stride + i], lo[2 * stride + i], hi[i], hi[stride + i], hi[2 * stride + i]);
    const BV r = sdfk_box_run<NC, NV>(code, n_instr, prm, fac, tab, result_reg, start);
    out_lo[i] = r.lo;
    out_hi[i] = r.hi;
}

// ---- octree refinement --------------------------------------------------------------------------------------------
struct SdfkBoxDomain {
    double lo[3], hi[3];
};
// what the refinement kernel accumulates: children needed, boxes per status, integer hull of the boxes not outside
struct SdfkBoxStats {
    unsigned long long needed, inside, outside, mixed;
    int mn[3], mx[3];
};

// fp32 values not above / not below a double
SDFK_DEV float sdfk_f32_below(double x) {
    float f = (float)x;
    if ((double)f > x) {
        const unsigned u = __builtin_bit_cast(unsigned, f);
        f = (f > 0.0f) ? __builtin_bit_cast(float, u - 1u) : ((f < 0.0f) ? __builtin_bit_cast(float, u + 1u) : __builtin_bit_cast(float, 0x80000001u));
    }
    return f;
}
SDFK_DEV float sdfk_f32_above(double x) { return -sdfk_f32_below(-x); }
// ends of cell i of 2^level along one axis of the domain, in float64 (the last cell ends at the domain's end exactly)
SDFK_DEV void sdfk_key_ends(double dlo, double dhi, unsigned i, int level, double* lo, double* hi) {
    const double scale = 1.0 / (double)(1u << level);
    const double w = dhi - dlo;
    *lo = dlo + w * ((double)i * scale);
    *hi = (i + 1u == (1u << level)) ? dhi : dlo + w * ((double)(i + 1u) * scale);
}

template <int NC, int NV>
__global__ __launch_bounds__(SDFK_BLOCK) void sdfk_enclose_octree_kernel(
    const uint2* __restrict__ code, int n_instr, const float* __restrict__ prm, const float* __restrict__ fac,
    const float* __restrict__ tab, int result_reg, const unsigned long long* __restrict__ keys, long long n, SdfkBoxDomain dom,
    int dims, float level, signed char* __restrict__ status, unsigned long long* __restrict__ children, long long capacity,
    SdfkBoxStats* __restrict__ stats) {
    const long long i = (long long)sdfk_bx() * SDFK_BLOCK + sdfk_tx();
    const unsigned lane = sdfk_tx() & 63u;
    const bool live = i < n;                            // no early return: the whole wave ballots below
    const unsigned long long key = live ? keys[i] : 0ull;
    const int lv = (int)(key >> (3 * SDFK_BOX_KEY_BITS));
    const unsigned ix = (unsigned)((key >> (2 * SDFK_BOX_KEY_BITS)) & SDFK_BOX_KEY_MASK);
    const unsigned iy = (unsigned)((key >> SDFK_BOX_KEY_BITS) & SDFK_BOX_KEY_MASK), iz = (unsigned)(key & SDFK_BOX_KEY_MASK);
    double l0, h0, l1, h1, l2 = 0.0, h2 = 0.0;
    sdfk_key_ends(dom.lo[0], dom.hi[0], ix, lv, &l0, &h0);
    sdfk_key_ends(dom.lo[1], dom.hi[1], iy, lv, &l1, &h1);
    if (dims == 3) sdfk_key_ends(dom.lo[2], dom.hi[2], iz, lv, &l2, &h2);
    const BC start = sdfk_box_start(sdfk_f32_below(l0), sdfk_f32_below(l1), sdfk_f32_below(l2), sdfk_f32_above(h0),
                                    sdfk_f32_above(h1), sdfk_f32_above(h2));
    const BV r = sdfk_box_run<NC, NV>(code, n_instr, prm, fac, tab, result_reg, start);
    const int st = (r.hi <= level) ? -1 : ((r.lo > level) ? 1 : 0);
    if (live && status) status[i] = (signed char)st;
    const bool in = live && st < 0, out = live && st > 0, mix = live && st == 0;
    const unsigned long long mmix = __ballot(mix);
    const unsigned nch = (dims == 3) ? 8u : 4u;
    const unsigned nmix = (unsigned)__popcll(mmix);
    // integer hull of the LEAVES that are not outside, per wave: inside boxes, and mixed ones where no child list is kept
    const bool leaf = in || (mix && !children);
    int mn0 = leaf ? (int)ix : 0x7fffffff, mn1 = leaf ? (int)iy : 0x7fffffff, mn2 = leaf ? (int)iz : 0x7fffffff;
    int mx0 = leaf ? (int)ix : -1, mx1 = leaf ? (int)iy : -1, mx2 = leaf ? (int)iz : -1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        mn0 = min(mn0, __shfl_xor(mn0, o)), mn1 = min(mn1, __shfl_xor(mn1, o)), mn2 = min(mn2, __shfl_xor(mn2, o));
        mx0 = max(mx0, __shfl_xor(mx0, o)), mx1 = max(mx1, __shfl_xor(mx1, o)), mx2 = max(mx2, __shfl_xor(mx2, o));
    }
    const unsigned nin = (unsigned)__popcll(__ballot(in)), nout = (unsigned)__popcll(__ballot(out));
    unsigned long long base = 0ull;
    if (lane == 0) {
        if (nmix) base = atomicAdd(&stats->needed, (unsigned long long)nmix * nch);      // one atomic per wave for the list
        if (nin) atomicAdd(&stats->inside, (unsigned long long)nin);
        if (nout) atomicAdd(&stats->outside, (unsigned long long)nout);
        if (nmix) atomicAdd(&stats->mixed, (unsigned long long)nmix);
        if (mx0 >= 0) {
            atomicMin(&stats->mn[0], mn0), atomicMin(&stats->mn[1], mn1), atomicMin(&stats->mn[2], mn2);
            atomicMax(&stats->mx[0], mx0), atomicMax(&stats->mx[1], mx1), atomicMax(&stats->mx[2], mx2);
        }
    }
    const unsigned blo = __builtin_amdgcn_readfirstlane((unsigned)base), bhi = __builtin_amdgcn_readfirstlane((unsigned)(base >> 32));
    base = ((unsigned long long)bhi << 32) | blo;
    if (mix && children) {
        const unsigned before = (unsigned)__popcll(mmix & ((1ull << lane) - 1ull));
        const unsigned long long pos = base + (unsigned long long)before * nch;
        if (pos + nch <= (unsigned long long)capacity) {              // never past the capacity: the host sees `needed`
            const unsigned long long up = (unsigned long long)(lv + 1) << (3 * SDFK_BOX_KEY_BITS);
            for (unsigned k = 0; k < nch; ++k) {
                const unsigned long long cx = 2ull * ix + (k & 1u), cy = 2ull * iy + ((k >> 1) & 1u), cz = (dims == 3) ? 2ull * iz + (k >> 2) : 0ull;
                children[pos + k] = up | (cx << (2 * SDFK_BOX_KEY_BITS)) | (cy << SDFK_BOX_KEY_BITS) | cz;
            }
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------
extern "C" int sdfk_box_pad_ulps(void) { return SDFK_BOX_PAD_ULPS; }

extern "C" int sdfk_box_has_rule(int op) {
    switch (op) {
#define SDFK_BOX_HAS(NAME, KIND, FN) case SDFK_OP_##NAME:
        SDFK_BOX_TABLE(SDFK_BOX_HAS)
#undef SDFK_BOX_HAS
        return 1;
        default:
            return 0;
    }
}

extern "C" int sdfk_program_box_check(sdfk_program* p, int* first_bad_op) {
    if (!p) return fail(-1, "null program");
    if (first_bad_op) *first_bad_op = -1;
    const size_t n_instr = p->code.size() / 2;
    for (size_t i = 0; i < n_instr; ++i) {
        const unsigned op = p->code[2 * i] & 255u;
        if (!sdfk_box_has_rule((int)op)) {
            if (first_bad_op) *first_bad_op = (int)i;
            char buf[160];
            snprintf(buf, sizeof buf, "instruction %zu (%s): no box rule", i, g_ops[op].name);
            g_err = buf;
            return 1;
        }
    }
    int nc = 0, nv = 0;
    dual_regs(p, &nc, &nv);
    if (nc > SDFK_DUAL_NC || nv > SDFK_DUAL_NV) {
        g_err = "program too large for the enclosure kernel";
        return 2;
    }
    return 0;
}

// the checks and the residency every enclosure launch shares
static int box_prepare(sdfk_program* p, const char* who, void* stream, LaunchCtx* x) {
    if (!p) return fail(-1, "null program");
    int bad = -1;
    const int chk = sdfk_program_box_check(p, &bad);
    if (chk) return fail(chk < 0 ? chk : -3, std::string(who) + ": " + g_err);
    return launch_ctx(p, stream, x);
}

extern "C" int sdfk_enclose_boxes_device(sdfk_program* p, const float* d_lo, const float* d_hi, int64_t n, int64_t stride,
                                         const float* d_factors, float* d_out_lo, float* d_out_hi, void* stream) {
    if (n < 0 || stride < n) return fail(-1, "sdfk_enclose_boxes_device: row stride smaller than the box count");
    if (n > 0 && (!d_lo || !d_hi || !d_factors || !d_out_lo || !d_out_hi))
        return fail(-1, "sdfk_enclose_boxes_device: null device pointer");
    LaunchCtx x;
    const int rc = box_prepare(p, "sdfk_enclose_boxes_device", stream, &x);
    if (rc) return rc;
    if (n == 0) return 0;
    const unsigned blocks = (unsigned)((n + SDFK_BLOCK - 1) / SDFK_BLOCK);
#define SDFK_ENCLOSE_GO(NC, NV) hipLaunchKernelGGL((sdfk_enclose_kernel<NC, NV>), dim3(blocks), dim3(SDFK_BLOCK), 0, x.stream, x.d->d_code, \
                                                   x.n_instr, x.prm, d_factors, x.tab, d_lo, d_hi, (long long)stride, (long long)n,    \
                                                   d_out_lo, d_out_hi, x.result_reg)
    SDFK_REGFILE(p, SDFK_DUAL_NC, SDFK_DUAL_NV, SDFK_ENCLOSE_GO);
#undef SDFK_ENCLOSE_GO
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" size_t sdfk_enclose_octree_scratch(void) { return sizeof(SdfkBoxStats); }

extern "C" int sdfk_enclose_octree_device(sdfk_program* p, const uint64_t* d_keys, int64_t n, const double* domain, int dims,
                                          float level, const float* d_factors, signed char* d_status, uint64_t* d_children,
                                          int64_t capacity, int64_t* needed, int64_t* counts, int* hull, void* d_scratch,
                                          void* stream) {
    if (n < 0 || capacity < 0 || (dims != 2 && dims != 3)) return fail(-1, "sdfk_enclose_octree_device: bad sizes");
    if (!domain || !needed || !counts || !hull || !d_scratch) return fail(-1, "sdfk_enclose_octree_device: null pointer");
    if (n > 0 && (!d_keys || !d_factors)) return fail(-1, "sdfk_enclose_octree_device: null device pointer");
    if (capacity > 0 && !d_children) return fail(-1, "sdfk_enclose_octree_device: a capacity without a list");
    SdfkBoxDomain dom;
    for (int a = 0; a < 3; ++a) {
        dom.lo[a] = a < dims ? domain[a] : 0.0;
        dom.hi[a] = a < dims ? domain[3 + a] : 0.0;
        if (!(std::isfinite(dom.lo[a]) && std::isfinite(dom.hi[a]) && dom.lo[a] <= dom.hi[a]))
            return fail(-1, "sdfk_enclose_octree_device: the domain must be finite and ordered");
    }
    LaunchCtx x;
    const int rc = box_prepare(p, "sdfk_enclose_octree_device", stream, &x);
    if (rc) return rc;
    hipStream_t s = x.stream;
    SdfkBoxStats st = {};
    for (int a = 0; a < 3; ++a) st.mn[a] = 0x7fffffff, st.mx[a] = -1;
    if (n > 0) {
        HIPCHK(hipMemcpyAsync(d_scratch, &st, sizeof st, hipMemcpyHostToDevice, s));
        const unsigned blocks = (unsigned)((n + SDFK_BLOCK - 1) / SDFK_BLOCK);
#define SDFK_OCTREE_GO(NC, NV) hipLaunchKernelGGL((sdfk_enclose_octree_kernel<NC, NV>), dim3(blocks), dim3(SDFK_BLOCK), 0, s, x.d->d_code, \
                                                  x.n_instr, x.prm, d_factors, x.tab, x.result_reg, (const unsigned long long*)d_keys, \
                                                  (long long)n, dom, dims, level, d_status,                                      \
                                                  (unsigned long long*)(capacity > 0 ? d_children : nullptr), (long long)capacity, \
                                                  (SdfkBoxStats*)d_scratch)
        SDFK_REGFILE(p, SDFK_DUAL_NC, SDFK_DUAL_NV, SDFK_OCTREE_GO);
#undef SDFK_OCTREE_GO
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&st, d_scratch, sizeof st, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    *needed = (int64_t)st.needed;
    counts[0] = (int64_t)st.inside, counts[1] = (int64_t)st.outside, counts[2] = (int64_t)st.mixed;
    for (int a = 0; a < 3; ++a) hull[a] = st.mn[a], hull[3 + a] = st.mx[a];
    return 0;
}
