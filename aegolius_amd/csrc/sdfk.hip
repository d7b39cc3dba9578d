// sdfk.hip — kernels and C-ABI of libsdfk.so (gfx950 only).
//
//   * sdfk_interp_kernel<VEC,SRC> : generic register-machine interpreter. The program and its
//     parameters are wave-uniform, so the dispatch runs on the scalar unit (s_load of the
//     instruction word, scalar branch) and parameters arrive in SGPRs through the scalar cache.
//   * specialised kernels        : the same per-point functions (sdfk_device.h) called in
//     straight-line order, generated per tree TOPOLOGY (parameters stay runtime data) by
//     sdfk_codegen.cpp, compiled with hiprtc on first use and cached per (device, topology).
//   * access pattern             : one thread owns 4 consecutive points — three 16-byte loads
//     (x, y, z rows of the (3,N) array), one 16-byte store; a wave covers 1 KiB per row per
//     instruction, fully coalesced. Algorithmic traffic 16 B/point.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared (see __graft_entry__.build()).
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <chrono>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <string>
#include <variant>
#include <vector>
#include <dirent.h>
#include <dlfcn.h>
#include <fcntl.h>
#include <signal.h>
#include <spawn.h>
#include <sys/wait.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/time.h>
#include <unistd.h>

#include "../../include/sdfk.h"
#include "sdfk_device.h"
#include "sdfk_access.h"
#include "sdfk_codegen.h"

// ------------------------------------------------------------------------------------------------
// opcode tables from the single source of truth
// ------------------------------------------------------------------------------------------------
enum {
#define SDFK_OP(NAME, KIND, NP, FUNC) SDFK_OP_##NAME,
#include "sdfk_ops.def"
#undef SDFK_OP
    SDFK_OP_COUNT
};

static const sdfk_opinfo g_ops[] = {
#define SDFK_OP(NAME, KIND, NP, FUNC) {#NAME, SDFK_KIND_##KIND, NP, #FUNC},
#include "sdfk_ops.def"
#undef SDFK_OP
};

extern "C" const sdfk_opinfo* sdfk_op_table(int* count) {
    if (count) *count = SDFK_OP_COUNT;
    return g_ops;
}

// interpreter register-file limits (the specialised path has none beyond the 8-bit operand fields)
#define SDFK_NC 8
#define SDFK_NV 8
// six programs in seven need at most 2 coordinate and 3 value registers (every BASELINE config does): that register
// file fits the VGPRs, the full one lives in scratch
#define SDFK_NC_SMALL 2
#define SDFK_NV_SMALL 3

// ------------------------------------------------------------------------------------------------
// interpreter kernel
// ------------------------------------------------------------------------------------------------
template <int VEC, int NC, int NV, typename SRC>
__global__ __launch_bounds__(SDFK_BLOCK) void sdfk_interp_kernel(const uint2* __restrict__ code, int n_instr,
                                                                const float* __restrict__ prm,
                                                                const float* __restrict__ tab, SRC src, long long off,
                                                                long long n, float* __restrict__ out, int result_reg,
                                                                const float* __restrict__ aux, long long aux_stride) {
    const long long block_base = (long long)sdfk_bx() * (SDFK_BLOCK * VEC);
    const unsigned lane_off = sdfk_tx() * VEC;
    if (block_base + lane_off >= n) return;
    // Register files indexed by the (wave-uniform) register number. The small coordinate file is three plain float
    // arrays, which the compiler keeps in VGPRs next to V; the full-size one is an array of structs and lives in
    // scratch — as plain arrays it takes 173 VGPRs, two waves per SIMD, and is slower (52.7 against 44.7 ms on the
    // north-star tree). (Wrapping either in a struct sends V to scratch as well: 62 ms.)
    constexpr bool SPLIT = NC <= SDFK_NC_SMALL;
    float CX[SPLIT ? NC : 1][VEC], CY[SPLIT ? NC : 1][VEC], CZ[SPLIT ? NC : 1][VEC];
    V3 CS[SPLIT ? 1 : NC][VEC];
    float V[NV][VEC];
#define SDFK_CGET(r, v) (SPLIT ? V3{CX[SPLIT ? (r) : 0][v], CY[SPLIT ? (r) : 0][v], CZ[SPLIT ? (r) : 0][v]} : CS[SPLIT ? 0 : (r)][v])
#define SDFK_CSET(r, v, q)                                                                      \
    do {                                                                                        \
        const V3 q_ = (q);                                                                      \
        if constexpr (SPLIT) { CX[SPLIT ? (r) : 0][v] = q_.x; CY[SPLIT ? (r) : 0][v] = q_.y; CZ[SPLIT ? (r) : 0][v] = q_.z; } \
        else CS[SPLIT ? 0 : (r)][v] = q_;                                                       \
    } while (0)
    {
        V3 p0[VEC];
        sdfk_load<VEC>(src, off + block_base, lane_off, p0);
        _Pragma("unroll") for (int v = 0; v < VEC; ++v) SDFK_CSET(0, v, p0[v]);
    }
    uint2 fetched = code[0];         // wave-uniform -> scalar load; the next word is requested before this one executes
    for (int pc = 0; pc < n_instr; ++pc) {
        const uint2 ins = fetched;
        fetched = code[min(pc + 1, n_instr - 1)];
        const unsigned op = ins.x & 255u, a = (ins.x >> 8) & 255u, b = (ins.x >> 16) & 255u, c = ins.x >> 24;
        const float* __restrict__ P = prm + ins.y;
        if (op == SDFK_OP_V_FIELD) {   // auxiliary field c at this lane's points (validated: aux != nullptr)
            _Pragma("unroll") for (int v = 0; v < VEC; ++v)
                V[a][v] = sdfk_aux<float>(aux + off + block_base + lane_off + v, aux_stride, (int)c);
            continue;
        }
        switch (op) {
#define SDFK_EXEC_C_C(F) \
    _Pragma("unroll") for (int v = 0; v < VEC; ++v) SDFK_CSET(a, v, F(SDFK_CGET(b, v), P, tab, (int)c))
#define SDFK_EXEC_V_C(F) \
    _Pragma("unroll") for (int v = 0; v < VEC; ++v) V[a][v] = F(SDFK_CGET(b, v), P, tab)
#define SDFK_EXEC_V_V(F) \
    _Pragma("unroll") for (int v = 0; v < VEC; ++v) V[a][v] = F(V[b][v], P)
#define SDFK_EXEC_V_VV(F) \
    _Pragma("unroll") for (int v = 0; v < VEC; ++v) V[a][v] = F(V[b][v], V[c][v], P)
#define SDFK_OP(NAME, KIND, NP, FUNC) \
    case SDFK_OP_##NAME:              \
        SDFK_EXEC_##KIND(FUNC);       \
        break;
#include "sdfk_ops.def"
#undef SDFK_OP
            default:
                break;
        }
    }
    sdfk_store<VEC>(out, off + block_base + lane_off, V[result_reg]);
}

// (3,n) -> (n) streaming probe with the evaluation kernels' access pattern
__global__ __launch_bounds__(SDFK_BLOCK) void sdfk_probe_kernel(SrcArray src, long long n, float* __restrict__ out) {
    const long long block_base = (long long)sdfk_bx() * (SDFK_BLOCK * 4);
    const unsigned lane_off = sdfk_tx() * 4;
    if (block_base + lane_off >= n) return;
    V3 p[4];
    sdfk_load<4>(src, block_base, lane_off, p);
    float v[4] = {p[0].x + p[0].y + p[0].z, p[1].x + p[1].y + p[1].z, p[2].x + p[2].y + p[2].z,
                  p[3].x + p[3].y + p[3].z};
    sdfk_store<4>(out, block_base + lane_off, v);
}

__global__ __launch_bounds__(SDFK_BLOCK) void sdfk_gridfill_kernel(SrcGrid src, long long n, float* __restrict__ co,
                                                                  long long stride) {
    const long long block_base = (long long)sdfk_bx() * (SDFK_BLOCK * 4);
    const unsigned lane_off = sdfk_tx() * 4;
    const long long i = block_base + lane_off;
    if (i >= n) return;
    V3 p[4];
    sdfk_load<4>(src, block_base, lane_off, p);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        if (i + v < n) {
            co[i + v] = p[v].x;
            co[stride + i + v] = p[v].y;
            co[2 * stride + i + v] = p[v].z;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;
static int g_default_mode = SDFK_MODE_AUTO;

static int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            (void)hipGetLastError(); /* the runtime keeps it: the next launch check would see it */ \
            return fail(-100 - (int)e_, std::string(#expr) + ": " + hipGetErrorString(e_));       \
        }                                                                                         \
    } while (0)

// candidate lists of one evaluation in flight (chain mode, csrc/sdfk_codegen.cpp "sdfk_spec_cells"): cell spheres, list
// spans, the pool the lists are allocated from and its head — one set per STREAM, because calls on different streams
// (the two slots of the host pipeline) run side by side on one program
struct CellScratch {
    char* buf = nullptr;
    size_t bytes = 0;
};
struct DevState {
    uint2* d_code = nullptr;
    float* d_params = nullptr;
    float* d_tables = nullptr;
    float* d_ptan0 = nullptr;  // 3 rows of zero parameter tangents (sdfk_project.inc), made on first use
    unsigned long long params_version = 0;
    std::map<hipStream_t, CellScratch> cells;
};

// One hiprtc translation unit = (program topology, kernel flavour, build options). The code object is built once
// per PROCESS — by whichever thread asks first, outside every global lock — and shared by all devices; a device
// only loads it (hipModuleLoadData). state: 0 idle, 1 building, 2 ready, 3 failed.
struct CodeObject {
    std::mutex mu;
    std::condition_variable cv;
    int state = 0;
    std::vector<char> co;
    std::string error;
    std::string disk_path;                // non-empty: `co` was read from this file of the on-disk cache
    double build_seconds = 0.0;
    std::chrono::steady_clock::time_point failed_at;
};
struct SpecModule {                   // a code object loaded on one device
    std::mutex mu;
    bool loaded = false, failed = false;
    hipModule_t mod = nullptr;
    hipFunction_t fn[4] = {nullptr, nullptr, nullptr, nullptr};   // ([2], [3]: the culled pair of the ray / span flavours)
    std::string error;
};

struct sdfk_program {
    std::vector<uint32_t> code;  // 2 words / instruction
    std::vector<float> params, tables;
    int result_reg = 0;
    bool interp_ok = true;  // fits the interpreter's register file
    bool interp_small = false;  // ... and its small instantiation (SDFK_NC_SMALL coordinate / SDFK_NV_SMALL value registers)
    int n_aux = 0;          // auxiliary per-point fields read by V_FIELD instructions
    unsigned long long params_version = 1;
    std::string key;
    std::string source;
    std::vector<sdfk_cullsite> sites;  // brick-culling sites the mask kernels use: the SDFK_MASK_SITES widest (sdfk_program_set_cull)
    std::vector<sdfk_cullsite> sites_all;  // every site that was passed in
    bool chain_mode = false;           // long n-ary min / max chain: table-driven kernels (sdfk_codegen.cpp)
    int chain_members = 0;             // its members (the program may hold more sites: combiners above the chain)
    std::mutex mu;
    std::map<int, DevState> dev;
};

static std::mutex g_code_mu;                                    // guards the two maps only, never a build
static std::map<std::string, std::shared_ptr<CodeObject>> g_code;
static std::map<std::pair<int, std::string>, std::shared_ptr<SpecModule>> g_mods;

extern "C" int sdfk_abi_version(void) { return SDFK_ABI_VERSION; }

extern "C" int sdfk_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

extern "C" const char* sdfk_last_error(void) { return g_err.c_str(); }
#define SDFK_MASK_SITES 512   // sites a row-block kernel carries skip bits for (16 words of 64 bits per brick at most)
extern "C" void sdfk_set_default_mode(int mode) { g_default_mode = mode; }

// ---- validation -------------------------------------------------------------------------------
static int table_rows_ok(const sdfk_program* p, int op, const float* P, std::string* why) {
    auto bad = [&](const char* m) {
        *why = m;
        return 0;
    };
    long long cnt = (long long)P[0], off = (long long)P[1];
    if (op == SDFK_OP_P_POLYSIGN && P[0] == -1.0f) cnt = 1;      // one piece, raw side value (interior_convex)
    else if (!(P[0] >= 0.0f) || (float)cnt != P[0]) return bad("table count/offset not integral");
    if (!(P[1] >= 0.0f) || (float)off != P[1]) return bad("table count/offset not integral");
    long long nt = (long long)p->tables.size();
    long long row = 0;
    switch (op) {
        case SDFK_OP_P_SEGLINE3: row = 7; break;
        case SDFK_OP_P_NEAREST3: row = 3; break;
        case SDFK_OP_P_SEGLINE2: row = 5; break;
        case SDFK_OP_P_NEAREST2: row = 2; break;
        case SDFK_OP_P_SHAPESIGN: row = 6; break;
        case SDFK_OP_CURVEINST: row = (P[2] != 0.0f) ? 12 : 3; break;
        case SDFK_OP_CURVEINSTT:
        case SDFK_OP_P_NEARTREE: {
            // every index the kernel will follow stays inside the table; no box is empty (root -> middle -> leaf -> points)
            if (cnt < 1) return bad("point tree without root boxes");
            if (op == SDFK_OP_P_NEARTREE && P[2] != 2.0f && P[2] != 3.0f) return bad("point tree dimension must be 2 or 3");
            if (off + 8 * cnt > nt) return bad("point tree: root boxes out of range");
            const float* t = p->tables.data() + off;
            const long long room = nt - off;
            auto kids = [&](const float* box, long long width, long long* first, long long* n) {
                const float ff = box[6], fn = box[7];
                *first = (long long)ff;
                *n = (long long)fn;
                return ff >= 0.0f && fn >= 1.0f && (float)*first == ff && (float)*n == fn && *first + width * *n <= room;
            };
            for (long long r = 0; r < cnt; ++r) {
                long long mfirst, nm;
                if (!kids(t + 8 * r, 8, &mfirst, &nm)) return bad("point tree: middle boxes out of range");
                for (long long i = 0; i < nm; ++i) {
                    long long first, nl;
                    if (!kids(t + mfirst + 8 * i, 8, &first, &nl)) return bad("point tree: leaf boxes out of range");
                    for (long long l = 0; l < nl; ++l) {
                        long long pfirst, pcount;
                        if (!kids(t + first + 8 * l, 3, &pfirst, &pcount)) return bad("point tree: points out of range");
                        if (op == SDFK_OP_CURVEINSTT) {
                            // the original index of every point the kernel can pick is readable and names a row inside the table
                            const long long base = (long long)P[4], rows = (long long)P[3], ids = (long long)P[5];
                            const long long stride = (P[2] != 0.0f) ? 12 : 3;
                            if (!(P[3] >= 0.0f) || !(P[4] >= 0.0f) || !(P[5] >= 0.0f) || (float)base != P[4] || (float)rows != P[3] ||
                                (float)ids != P[5] || pfirst < base || (pfirst - base) % 3 != 0 ||
                                ids + (pfirst - base) / 3 + pcount > nt)
                                return bad("instancing tree: original indices out of range");
                            for (long long q = 0; q < pcount; ++q) {
                                const float of = p->tables[(size_t)(ids + (pfirst - base) / 3 + q)];
                                const long long o = (long long)of;
                                if (!(of >= 0.0f) || (float)o != of || rows + (o + 1) * stride > nt)
                                    return bad("instancing tree: instance row out of range");
                            }
                        }
                    }
                }
            }
            return 1;
        }
        case SDFK_OP_P_POLYSIGN: {
            long long pos = off;
            for (long long j = 0; j < cnt; ++j) {
                if (pos >= nt) return bad("polygon piece header out of range");
                float kf = p->tables[pos];
                long long k = (long long)kf;
                if (!(kf >= 0.0f) || (float)k != kf) return bad("polygon piece size not integral");
                pos += 1 + 4 * k;
                if (pos > nt) return bad("polygon piece out of range");
            }
            return 1;
        }
        default: return 1;
    }
    if (off + cnt * row > nt) return bad("table rows out of range");
    if (op == SDFK_OP_CURVEINST && cnt < 1) return bad("curve instancing needs at least one instance");
    return 1;
}

static bool is_table_op(int op) {
    return op == SDFK_OP_P_SEGLINE3 || op == SDFK_OP_P_NEAREST3 || op == SDFK_OP_P_SEGLINE2 ||
           op == SDFK_OP_P_NEAREST2 || op == SDFK_OP_CURVEINST || op == SDFK_OP_P_POLYSIGN || op == SDFK_OP_P_NEARTREE ||
           op == SDFK_OP_CURVEINSTT ||
           op == SDFK_OP_P_SHAPESIGN;
}

static int validate(sdfk_program* p, std::string* why) {
    const size_t n_instr = p->code.size() / 2;
    std::vector<char> cdef(256, 0), vdef(256, 0);
    cdef[0] = 1;  // C0 = input point
    unsigned max_c = 0, max_v = 0;
    char buf[160];
    for (size_t i = 0; i < n_instr; ++i) {
        const uint32_t w = p->code[2 * i], poff = p->code[2 * i + 1];
        const unsigned op = w & 255u, a = (w >> 8) & 255u, b = (w >> 16) & 255u, c = w >> 24;
        if (op >= SDFK_OP_COUNT) {
            snprintf(buf, sizeof buf, "instruction %zu: unknown opcode %u", i, op);
            *why = buf;
            return 0;
        }
        const sdfk_opinfo& info = g_ops[op];
        if ((size_t)poff + (size_t)info.nparams > p->params.size()) {
            snprintf(buf, sizeof buf, "instruction %zu (%s): parameters out of range", i, info.name);
            *why = buf;
            return 0;
        }
        bool ok = true;
        switch (info.kind) {
            case SDFK_KIND_C_C: ok = cdef[b]; cdef[a] = 1; max_c = std::max(max_c, std::max(a, b)); break;
            case SDFK_KIND_V_C: ok = cdef[b]; vdef[a] = 1; max_c = std::max(max_c, b); max_v = std::max(max_v, a); break;
            case SDFK_KIND_V_V: ok = vdef[b]; vdef[a] = 1; max_v = std::max(max_v, std::max(a, b)); break;
            case SDFK_KIND_V_VV:
                ok = vdef[b] && vdef[c];
                vdef[a] = 1;
                max_v = std::max(max_v, std::max(a, std::max(b, c)));
                break;
        }
        if (!ok) {
            snprintf(buf, sizeof buf, "instruction %zu (%s): reads a register that was never written", i, info.name);
            *why = buf;
            return 0;
        }
        if (op == SDFK_OP_V_FIELD) {
            if (c >= 32) {
                snprintf(buf, sizeof buf, "instruction %zu: auxiliary field index %u out of range (32)", i, c);
                *why = buf;
                return 0;
            }
            p->n_aux = std::max(p->n_aux, (int)c + 1);
        }
        if (op == SDFK_OP_SYMMETRY && c > 2) {
            snprintf(buf, sizeof buf, "instruction %zu: symmetry axis %u out of range", i, c);
            *why = buf;
            return 0;
        }
        if (is_table_op((int)op)) {
            std::string w2;
            if (!table_rows_ok(p, (int)op, p->params.data() + poff, &w2)) {
                snprintf(buf, sizeof buf, "instruction %zu (%s): %s", i, info.name, w2.c_str());
                *why = buf;
                return 0;
            }
        }
    }
    if (p->result_reg < 0 || p->result_reg > 255 || !vdef[p->result_reg]) {
        *why = "result register is never written";
        return 0;
    }
    p->interp_ok = (max_c < SDFK_NC) && (max_v < SDFK_NV) && (p->result_reg < SDFK_NV);
    p->interp_small = (max_c < SDFK_NC_SMALL) && (max_v < SDFK_NV_SMALL) && (p->result_reg < SDFK_NV_SMALL);
    return 1;
}

extern "C" sdfk_program* sdfk_program_create(const uint32_t* code, size_t n_instr, const float* params,
                                             size_t n_params, const float* tables, size_t n_tables, int result_reg) {
    if (!code || n_instr == 0 || n_instr > (1u << 20)) {
        fail(-1, "sdfk_program_create: empty or oversized program");
        return nullptr;
    }
    std::unique_ptr<sdfk_program> p(new sdfk_program);
    p->code.assign(code, code + 2 * n_instr);
    if (params && n_params) p->params.assign(params, params + n_params);
    if (tables && n_tables) p->tables.assign(tables, tables + n_tables);
    p->result_reg = result_reg;
    std::string why;
    if (!validate(p.get(), &why)) {
        fail(-2, "sdfk_program_create: " + why);
        return nullptr;
    }
    p->key.assign(reinterpret_cast<const char*>(p->code.data()), p->code.size() * sizeof(uint32_t));
    p->key.push_back((char)result_reg);
    return p.release();
}

static void free_dev_state(sdfk_program* p) {
    int cur = 0;
    bool have = hipGetDevice(&cur) == hipSuccess;
    for (auto& kv : p->dev) {
        if (hipSetDevice(kv.first) != hipSuccess) continue;
        if (kv.second.d_code) (void)hipFree(kv.second.d_code);
        if (kv.second.d_params) (void)hipFree(kv.second.d_params);
        if (kv.second.d_tables) (void)hipFree(kv.second.d_tables);
        if (kv.second.d_ptan0) (void)hipFree(kv.second.d_ptan0);
        for (auto& cs : kv.second.cells)
            if (cs.second.buf) (void)hipFree(cs.second.buf);
    }
    if (have) (void)hipSetDevice(cur);
    p->dev.clear();
}

extern "C" void sdfk_program_destroy(sdfk_program* p) {
    if (!p) return;
    free_dev_state(p);
    delete p;
}

extern "C" int sdfk_program_set_params(sdfk_program* p, const float* params, size_t n_params) {
    if (!p) return fail(-1, "null program");
    std::lock_guard<std::mutex> lk(p->mu);
    if (n_params != p->params.size()) return fail(-2, "sdfk_program_set_params: parameter count differs from the program's");
    std::vector<float> old = p->params;
    p->params.assign(params, params + n_params);
    std::string why;
    if (!validate(p, &why)) {  // table counts / offsets live in the parameters
        p->params = old;
        return fail(-2, "sdfk_program_set_params: " + why);
    }
    p->params_version++;
    return 0;
}

// ---- brick culling sites ---------------------------------------------------------------------
static void instr_fields(const sdfk_program* p, size_t i, unsigned* op, unsigned* a, unsigned* b, unsigned* c) {
    const uint32_t w = p->code[2 * i];
    *op = w & 255u; *a = (w >> 8) & 255u; *b = (w >> 16) & 255u; *c = w >> 24;
}

// May the instructions [lo, hi] be skipped when the combiner `comb` does not need the value they
// produce? Only if nothing executed later reads a register they would have written.
static bool range_skippable(const sdfk_program* p, uint32_t lo, uint32_t hi, uint32_t comb, unsigned result_vreg) {
    const size_t n = p->code.size() / 2;
    std::vector<char> wc(256, 0), wv(256, 0);
    unsigned op, a, b, c;
    for (size_t i = lo; i <= hi; ++i) {
        instr_fields(p, i, &op, &a, &b, &c);
        (g_ops[op].kind == SDFK_KIND_C_C ? wc : wv)[a] = 1;
    }
    instr_fields(p, hi, &op, &a, &b, &c);
    if (g_ops[op].kind == SDFK_KIND_C_C || a != result_vreg) return false;  // range must end by producing the operand
    for (size_t j = hi + 1; j < n; ++j) {
        instr_fields(p, j, &op, &a, &b, &c);
        const int kind = g_ops[op].kind;
        if (kind == SDFK_KIND_C_C || kind == SDFK_KIND_V_C) {
            if (wc[b]) return false;
        } else if (kind == SDFK_KIND_V_V) {
            if (wv[b]) return false;
        } else {
            const bool is_comb = (j == comb);
            if (wv[b] && !(is_comb && b == result_vreg)) return false;
            if (wv[c] && !(is_comb && c == result_vreg)) return false;
        }
        (kind == SDFK_KIND_C_C ? wc : wv)[a] = 0;   // redefined: later reads see the new value
    }
    return !wv[(unsigned)p->result_reg];
}

static bool is_cullable_op(unsigned op) {
    return op == SDFK_OP_VMIN || op == SDFK_OP_VMAX || op == SDFK_OP_VSUBTRACT || op == SDFK_OP_SMIN2 ||
           op == SDFK_OP_SMIN3 || op == SDFK_OP_SMAX3 || op == SDFK_OP_SSUB3;
}

extern "C" int sdfk_program_set_cull(sdfk_program* p, const uint32_t* rows, size_t n_sites, const float* k) {
    if (!p) return fail(-1, "null program");
    if (n_sites > 32767) return fail(-2, "sdfk_program_set_cull: at most 32767 sites");
    if (n_sites && (!rows || !k)) return fail(-1, "sdfk_program_set_cull: null arrays");
    std::lock_guard<std::mutex> lk(p->mu);
    if (!p->source.empty() || !p->dev.empty())
        return fail(-2, "sdfk_program_set_cull: must be called before the program is first used");
    if (p->n_aux > 0) n_sites = 0;   // auxiliary fields have no Lipschitz bound and the culling kernels do not carry them
    const size_t n = p->code.size() / 2;
    std::vector<sdfk_cullsite> sites;
    for (size_t i = 0; i < n_sites; ++i) {
        sdfk_cullsite t{rows[5 * i], rows[5 * i + 1], rows[5 * i + 2], rows[5 * i + 3], rows[5 * i + 4], k[i], 0, 0};
        if (!(t.comb < n && t.a0 <= t.a1 && t.a1 + 1 == t.b0 && t.b0 <= t.b1 && t.b1 + 1 == t.comb))
            return fail(-2, "sdfk_program_set_cull: malformed site ranges");
        if (!(t.k >= 0.0f) || !std::isfinite(t.k)) return fail(-2, "sdfk_program_set_cull: bad Lipschitz sum");
        unsigned op, a, b, c;
        instr_fields(p, t.comb, &op, &a, &b, &c);
        if (!is_cullable_op(op)) return fail(-2, "sdfk_program_set_cull: site is not at a min/max-type combiner");
        if (i && rows[5 * i] <= rows[5 * (i - 1)]) return fail(-2, "sdfk_program_set_cull: sites must be sorted");
        for (const sdfk_cullsite& u : sites) {   // spans [a0, comb] nest or are disjoint
            const bool disjoint = u.comb < t.a0;
            const bool nested = u.a0 >= t.a0 && (u.comb <= t.a1 || (u.a0 >= t.b0 && u.comb <= t.b1));
            if (!disjoint && !nested) return fail(-2, "sdfk_program_set_cull: sites overlap without nesting");
        }
        t.skip_a_ok = range_skippable(p, t.a0, t.a1, t.comb, b) ? 1 : 0;
        t.skip_b_ok = range_skippable(p, t.b0, t.b1, t.comb, c) ? 1 : 0;
        sites.push_back(t);
    }
    // the row-block kernels carry two mask bits per site, 32 sites per 64-bit word and brick (SDFK_NMASK words; rounds 1-3:
    // two words, 64 sites — a left-deep union of 200 primitives then evaluated 135 of them at every point): up to
    // SDFK_MASK_SITES = 512 sites, the widest ones, in program order (the line-brick kernel picks its 31 among them)
    p->sites_all = sites;
    if (sites.size() > SDFK_MASK_SITES) {
        std::vector<size_t> order(sites.size());
        for (size_t i = 0; i < order.size(); ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) {
            return (sites[x].a1 - sites[x].a0) + (sites[x].b1 - sites[x].b0) > (sites[y].a1 - sites[y].a0) + (sites[y].b1 - sites[y].b0);
        });
        order.resize(SDFK_MASK_SITES);
        std::sort(order.begin(), order.end());
        std::vector<sdfk_cullsite> widest;
        for (size_t i : order) widest.push_back(sites[i]);
        sites.swap(widest);
    }
    p->sites = sites;
    p->chain_members = sdfk_chain_mode(g_ops, SDFK_OP_COUNT, p->code.data(), p->code.size() / 2, p->result_reg, p->sites_all);
    p->chain_mode = p->chain_members > 0;
    p->key.append("|cull");
    for (const sdfk_cullsite& t : p->sites_all) {
        p->key.append(reinterpret_cast<const char*>(&t), sizeof t);
    }
    return 0;
}

extern "C" const char* sdfk_program_source(sdfk_program* p) {
    if (!p) return nullptr;
    std::lock_guard<std::mutex> lk(p->mu);
    if (p->source.empty())
        p->source = sdfk_generate_source(g_ops, SDFK_OP_COUNT, p->code.data(), p->code.size() / 2, p->result_reg,
                                         p->sites, SDFK_FL_ALL, &p->sites_all);
    return p->source.c_str();
}

// launch geometry that the build options and the keys of code objects depend on (sdfk_launch.inc)
static int tile_waves();
static int tile_wbricks();
static int rows_geo(const sdfk_program* p);
#include "sdfk_jit.inc"
#include "sdfk_launch.inc"


static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// What the array entry points check before anything runs, and the request they hand to run(): device pointers, the row
// stride, the row length (min_row_len 1: the call has one; 0: it may pass none; -1: the call has no such argument), and
// whether rows and output allow 16-byte accesses.
static int array_entry(const char* who, sdfk_program* p, const float* d_co, int64_t n, int64_t row_stride, int64_t row_len,
                       int min_row_len, float* d_out, void* stream, int mode, SrcArray* a, EvalCall* c) {
    if (!d_co || !d_out) return fail(-1, std::string(who) + ": null device pointer");
    if (row_stride < n) return fail(-1, std::string(who) + ": row stride smaller than the point count");
    if (min_row_len >= 0 && (row_len < min_row_len || (row_len > 0 && n > 0 && n % row_len != 0)))
        return fail(-1, std::string(who) + ": the point count is not a multiple of the row length");
    *a = {d_co, (long long)row_stride};
    *c = array_call(p, a, n, d_out, stream, mode, aligned16(d_co) && aligned16(d_out) && (row_stride % 4 == 0));
    c->row_len = min_row_len >= 0 ? row_len : 0;
    return 0;
}

extern "C" int sdfk_eval_device(sdfk_program* p, const float* d_co, int64_t n, int64_t row_stride, float* d_out,
                                void* stream, int mode) {
    SrcArray a;
    EvalCall c;
    const int rc = array_entry("sdfk_eval_device", p, d_co, n, row_stride, 0, -1, d_out, stream, mode, &a, &c);
    return rc ? rc : run(c);
}

extern "C" int sdfk_eval_device_rows(sdfk_program* p, const float* d_co, int64_t n, int64_t row_stride, int64_t row_len,
                                     float* d_out, void* stream, int mode) {
    SrcArray a;
    EvalCall c;
    const int rc = array_entry("sdfk_eval_device_rows", p, d_co, n, row_stride, row_len, 1, d_out, stream, mode, &a, &c);
    return rc ? rc : run(c);
}

/* include/sdfk.h: two coordinate rows, z = 0 by contract */
extern "C" int sdfk_eval_device_rows2d_xy(sdfk_program* p, const float* d_xy, int64_t n, int64_t row_stride, int64_t row_len,
                                          float* d_out, void* stream, int mode) {
    SrcArray a;
    EvalCall c;
    const int rc = array_entry("sdfk_eval_device_rows2d_xy", p, d_xy, n, row_stride, row_len, 0, d_out, stream, mode, &a, &c);
    if (rc) return rc;
    c.flat = row_len > 0;
    c.xy = true;
    return run(c);
}

extern "C" int sdfk_eval_device_rows3d(sdfk_program* p, const float* d_co, int64_t n, int64_t row_stride, int64_t row_len,
                                       int64_t plane_rows, int64_t first_row_in_plane, float* d_out, void* stream, int mode) {
    SrcArray a;
    EvalCall c;
    const int rc = array_entry("sdfk_eval_device_rows3d", p, d_co, n, row_stride, row_len, 1, d_out, stream, mode, &a, &c);
    if (rc) return rc;
    if (plane_rows < 0 || first_row_in_plane < 0 || (plane_rows > 0 && first_row_in_plane >= plane_rows))
        return fail(-1, "sdfk_eval_device_rows3d: plane_rows >= 0 and 0 <= first_row_in_plane < plane_rows");
    c.plane_rows = plane_rows;
    c.plane_phase = first_row_in_plane;
    return run(c);
}

extern "C" int sdfk_eval_device_rows2d(sdfk_program* p, const float* d_co, int64_t n, int64_t row_stride, int64_t row_len,
                                       float* d_out, void* stream, int mode) {
    SrcArray a;
    EvalCall c;
    const int rc = array_entry("sdfk_eval_device_rows2d", p, d_co, n, row_stride, row_len, 1, d_out, stream, mode, &a, &c);
    if (rc) return rc;
    c.flat = true;
    return run(c);
}

extern "C" int sdfk_eval_device_aux(sdfk_program* p, const float* d_co, int64_t n, int64_t row_stride, const float* d_aux,
                                    int n_aux, int64_t aux_stride, float* d_out, void* stream, int mode) {
    if (!p) return fail(-1, "sdfk_eval_device_aux: null pointer");
    SrcArray a;
    EvalCall c;
    const int rc = array_entry("sdfk_eval_device_aux", p, d_co, n, row_stride, 0, -1, d_out, stream, mode, &a, &c);
    if (rc) return rc;
    if (n_aux < p->n_aux) return fail(-1, "sdfk_eval_device_aux: the program reads more auxiliary fields than were passed");
    c.aux = d_aux;
    c.aux_stride = aux_stride;
    return run(c);
}

/* include/sdfk.h: the plan of a request, no device touched */
extern "C" int sdfk_debug_eval_plan(sdfk_program* p, const int64_t* request, int64_t* plan) {
    if (!p || !request || !plan) return fail(-1, "sdfk_debug_eval_plan: null argument");
    if (request[1] <= 0) return fail(-1, "sdfk_debug_eval_plan: the point count must be positive");
    if (request[0] && (request[10] < 1 || request[11] < 1 || request[12] < 0))
        return fail(-1, "sdfk_debug_eval_plan: grid sizes from 1, start from 0");
    SrcArray a = {nullptr, 0};
    SrcGrid g = {nullptr, nullptr, nullptr, (unsigned)request[10], (unsigned)request[11], (long long)request[12]};
    unsigned some_flags = 0;                                    // (the planner asks whether flags are written, not where)
    EvalCall c = request[0] ? grid_call(p, &g, request[1], nullptr, nullptr, (int)request[2], request[3] != 0)
                            : array_call(p, &a, request[1], nullptr, nullptr, (int)request[2], request[3] != 0);
    c.row_len = request[4];
    c.flat = request[5] != 0;
    c.plane_rows = request[6];
    c.plane_phase = request[7];
    if (request[8]) c.d_flags = &some_flags;
    c.xy = request[9] != 0;
    EvalPlan pl;
    const int rc = plan_eval(c, plan_env(), &pl);
    if (rc) return rc;
    plan[0] = pl.mode;
    plan[1] = pl.flavour;
    plan[2] = pl.needs_specialised ? 1 : 0;
    plan[3] = pl.rows() ? (int64_t)pl.rg.nbricks : 0;
    return 0;
}

extern "C" int sdfk_debug_row_masks(sdfk_program* p, const float* d_co, int64_t n, int64_t row_stride, int64_t row_len,
                                    uint64_t* d_masks, int64_t* n_bricks, int* brick_rows, void* stream_) {
    if (!p || !d_co) return fail(-1, "sdfk_debug_row_masks: null argument");
    if (p->sites.empty()) return fail(-2, "sdfk_debug_row_masks: program has no cull sites");
    if (p->chain_mode) return fail(-2, "sdfk_debug_row_masks: a chain-mode program keeps lists of surviving children, not mask words");
    RowGeom rg;
    if (row_stride < n || !rows_geometry(n, row_len, &rg))
        return fail(-1, "sdfk_debug_row_masks: the row-block kernel does not take this shape");
    if (n_bricks) *n_bricks = rg.nbricks;
    if (brick_rows) *brick_rows = 16;
    if (!d_masks) return 0;                      // size query
    LaunchCtx x;
    int rc = launch_ctx(p, stream_, &x);
    if (rc) return rc;
    std::shared_ptr<SpecModule> sk;
    rc = pick_kernel(p, x.device, SDFK_FL_ROWS_MASK, 0, SDFK_MODE_SPECIALIZED, false, "kernel", false, &sk);
    if (rc) return rc;
    long long stride = row_stride;
    void* args[] = {&x.prm, &x.tab, &d_co, &stride, &rg, &d_masks};
    const unsigned per_tile = (unsigned)(rows_waves(p) * rows_wbricks(p));
    HIPCHK(hipModuleLaunchKernel(sk->fn[0], (rg.nbricks + per_tile - 1) / per_tile, 1, 1, 64 * rows_waves(p), 1, 1, 0, x.stream,
                                 args, nullptr));
    return 0;
}

extern "C" int sdfk_debug_brick_masks(sdfk_program* p, const float* d_co, int64_t n, int64_t row_stride,
                                      uint64_t* d_masks, void* stream_) {
    if (!p || !d_co || !d_masks) return fail(-1, "sdfk_debug_brick_masks: null argument");
    if (!(aligned16(d_co) && row_stride % 4 == 0 && row_stride >= n && n > 0))
        return fail(-1, "sdfk_debug_brick_masks: needs 16-byte aligned rows");
    if (p->sites.empty()) return fail(-2, "sdfk_debug_brick_masks: program has no cull sites");
    if (p->chain_mode) return fail(-2, "sdfk_debug_brick_masks: chain-mode programs have no line-brick flavour");
    LaunchCtx x;
    int rc = launch_ctx(p, stream_, &x);
    if (rc) return rc;
    std::shared_ptr<SpecModule> sk;
    rc = pick_kernel(p, x.device, SDFK_FL_TILE_MASK, 0, SDFK_MODE_SPECIALIZED, false, "kernel", false, &sk);
    if (rc) return rc;
    long long stride = row_stride, nn = n;
    void* args[] = {&x.prm, &x.tab, &d_co, &stride, &nn, &d_masks};
    HIPCHK(hipModuleLaunchKernel(sk->fn[0], (unsigned)((n + tile_points() - 1) / tile_points()), 1, 1, tile_threads(),
                                 1, 1, 0, x.stream, args, nullptr));
    return 0;
}

// ---- grids -------------------------------------------------------------------------------------
extern "C" int sdfk_linspace_f32(double lo, double hi, int64_t n, float* out) {
    if (n < 0 || (n > 0 && !out)) return fail(-1, "sdfk_linspace_f32: bad arguments");
    if (n == 0) return 0;
    if (n == 1) {
        out[0] = (float)lo;
        return 0;
    }
    const double div = (double)(n - 1);
    const double delta = hi - lo;
    const double step = delta / div;
    for (int64_t i = 0; i < n; ++i) {
        // numpy: y = arange(n) * step + start  (step != 0) ; y = arange(n)/div * delta + start (step == 0)
        volatile double t = (step != 0.0) ? (double)i * step : ((double)i / div) * delta;
        out[i] = (float)(t + lo);
    }
    out[n - 1] = (float)hi;
    return 0;
}

struct AxisTables {
    float* d = nullptr;
    ~AxisTables() {
        if (d) (void)hipFree(d);
    }
};

static int upload_axes(const float* ax0, int64_t n0, const float* ax1, int64_t n1, const float* ax2, int64_t n2,
                       hipStream_t stream, AxisTables* t, SrcGrid* g, int64_t start) {
    if (!ax0 || !ax1 || !ax2 || n0 < 1 || n1 < 1 || n2 < 1) return fail(-1, "grid axes missing or empty");
    if (n1 > 0x7fffffff || n2 > 0x7fffffff) return fail(-1, "grid axis too long");
    HIPCHK(hipMalloc(&t->d, (size_t)(n0 + n1 + n2) * sizeof(float)));
    HIPCHK(hipMemcpyAsync(t->d, ax0, (size_t)n0 * sizeof(float), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(t->d + n0, ax1, (size_t)n1 * sizeof(float), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(t->d + n0 + n1, ax2, (size_t)n2 * sizeof(float), hipMemcpyHostToDevice, stream));
    g->ax0 = t->d;
    g->ax1 = t->d + n0;
    g->ax2 = t->d + n0 + n1;
    g->n1 = (unsigned)n1;
    g->n2 = (unsigned)n2;
    g->start = start;
    return 0;
}

extern "C" int sdfk_eval_grid_aux(sdfk_program* p, const float* ax0, int64_t n0, const float* ax1, int64_t n1,
                                  const float* ax2, int64_t n2, int64_t start, int64_t count, const float* d_aux, int n_aux,
                                  int64_t aux_stride, float* d_out, void* stream, int mode) {
    if (!p || !d_out) return fail(-1, "sdfk_eval_grid_aux: null pointer");
    if (start < 0 || count < 0 || start + count > n0 * n1 * n2) return fail(-1, "sdfk_eval_grid_aux: range outside the grid");
    if (n_aux < p->n_aux) return fail(-1, "sdfk_eval_grid_aux: the program reads more auxiliary fields than were passed");
    AxisTables t;
    SrcGrid g;
    int rc = upload_axes(ax0, n0, ax1, n1, ax2, n2, (hipStream_t)stream, &t, &g, start);
    if (rc) return rc;
    EvalCall c = grid_call(p, &g, count, d_out, stream, mode, aligned16(d_out));
    c.aux = d_aux;
    c.aux_stride = aux_stride;
    rc = run(c);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));  // the axis tables are freed on return
    return 0;
}
extern "C" int sdfk_eval_grid(sdfk_program* p, const float* ax0, int64_t n0, const float* ax1, int64_t n1,
                              const float* ax2, int64_t n2, int64_t start, int64_t count, float* d_out, void* stream,
                              int mode) {
    if (!d_out) return fail(-1, "sdfk_eval_grid: null output");
    if (start < 0 || count < 0 || start + count > n0 * n1 * n2) return fail(-1, "sdfk_eval_grid: range outside the grid");
    if (!p) return fail(-1, "null program");
    // (no auxiliary fields to pass: a program that reads some is refused by run(), as ever)
    return sdfk_eval_grid_aux(p, ax0, n0, ax1, n1, ax2, n2, start, count, nullptr, p->n_aux, 0, d_out, stream, mode);
}

// Host-buffer convenience for grids: evaluate flat indices [start, start+count) of the grid in device chunks
// and copy the field back; no coordinate array ever exists (host or device).
extern "C" int sdfk_eval_grid_host(sdfk_program* p, const float* ax0, int64_t n0, const float* ax1, int64_t n1,
                                   const float* ax2, int64_t n2, int64_t start, int64_t count, float* out, int device,
                                   int mode) {
    if (!p) return fail(-1, "null program");
    if (count < 0 || (count > 0 && !out)) return fail(-1, "sdfk_eval_grid_host: bad arguments");
    if (start < 0 || start + count > n0 * n1 * n2) return fail(-1, "sdfk_eval_grid_host: range outside the grid");
    if (count == 0) return 0;
    HIPCHK(hipSetDevice(device));
    int64_t chunk = std::min<int64_t>(count, (int64_t)1 << 27);   // 128 Mi points = 512 MiB of device memory
    const int64_t grow = n2 > 1 ? n2 : n1;                         // whole grid rows per chunk (row-block kernel)
    if (start % grow == 0 && chunk > grow) chunk = chunk / grow * grow;
    float* d_out = nullptr;
    HIPCHK(hipMalloc(&d_out, (size_t)chunk * sizeof(float)));
    AxisTables t;
    SrcGrid g;
    int rc = upload_axes(ax0, n0, ax1, n1, ax2, n2, nullptr, &t, &g, start);
    for (int64_t s = 0; s < count && rc == 0; s += chunk) {
        const int64_t m = std::min(chunk, count - s);
        g.start = start + s;
        rc = run(grid_call(p, &g, m, d_out, nullptr, mode, true));
        if (rc == 0 && hipMemcpy(out + s, d_out, (size_t)m * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(-6, "sdfk_eval_grid_host: device-to-host copy failed");
    }
    (void)hipFree(d_out);
    return rc;
}

// The partition both sharded calls share: the grid in n_shards slabs of whole rows, shard d on devices[d] (without a
// list: round-robin over the box), one host thread per shard running body(device, start, count). An error text is
// thread-local, so the first failing shard's is carried to the caller's thread.
template <typename Body>
static int for_each_shard(const char* who, const float* ax0, int64_t n0, const float* ax1, int64_t n1, const float* ax2,
                          int64_t n2, int n_shards, const int* devices, Body body) {
    if (n_shards < 1 || n_shards > 64) return fail(-1, std::string(who) + ": 1..64 shards");
    if (!ax0 || !ax1 || !ax2 || n0 < 1 || n1 < 1 || n2 < 1) return fail(-1, "grid axes missing or empty");
    const int n_dev = sdfk_device_count();
    if (n_dev < 1) return fail(-8, std::string(who) + ": no HIP device");
    for (int d = 0; d < n_shards; ++d) {
        const int dev = devices ? devices[d] : d % n_dev;
        if (dev < 0 || dev >= n_dev) return fail(-1, std::string(who) + ": device index out of range");
    }
    const int64_t total = n0 * n1 * n2, unit = n2 > 1 ? n2 : n1;
    const int64_t per = (total / unit / n_shards) * unit;
    std::vector<int> rc((size_t)n_shards, 0);
    std::vector<std::string> msg((size_t)n_shards);
    std::vector<std::thread> workers;
    for (int d = 0; d < n_shards; ++d) {
        const int dev = devices ? devices[d] : d % n_dev;
        const int64_t start = d * per, count = d < n_shards - 1 ? per : total - start;
        workers.emplace_back([=, &rc, &msg] {
            rc[(size_t)d] = count > 0 ? body(dev, start, count) : 0;
            if (rc[(size_t)d]) msg[(size_t)d] = sdfk_last_error();
        });
    }
    for (std::thread& t : workers) t.join();
    for (int d = 0; d < n_shards; ++d)
        if (rc[(size_t)d]) return fail(rc[(size_t)d], "shard " + std::to_string(d) + ": " + msg[(size_t)d]);
    return 0;
}

// One process, several devices: device d evaluates the d-th slab of whole grid rows and copies it into its part of
// the host field; the slabs run concurrently. The per-device state of a program and the kernel cache are keyed by
// device, so this is sdfk_eval_grid_host once per slab.
extern "C" int sdfk_eval_grid_sharded(sdfk_program* p, const float* ax0, int64_t n0, const float* ax1, int64_t n1,
                                      const float* ax2, int64_t n2, int n_shards, const int* devices, float* out,
                                      int mode) {
    if (!p || !out) return fail(-1, "sdfk_eval_grid_sharded: null argument");
    return for_each_shard("sdfk_eval_grid_sharded", ax0, n0, ax1, n1, ax2, n2, n_shards, devices,
                          [=](int dev, int64_t start, int64_t count) {
                              return sdfk_eval_grid_host(p, ax0, n0, ax1, n1, ax2, n2, start, count, out + start, dev, mode);
                          });
}

// The same partition with the field left ON THE DEVICES: shard d is evaluated on devices[d] and lands in its place of
// `d_full`, a buffer of n0 * n1 * n2 floats on `gather_device` — written in place by the shards that run on that device,
// moved by hipMemcpyPeerAsync (device to device over xGMI, no host buffer) by the others. A C consumer without torch gets
// the reassembled field on one GPU this way; the multi-process route with RCCL is aegolius_amd/distributed.py.
extern "C" int sdfk_eval_grid_sharded_device(sdfk_program* p, const float* ax0, int64_t n0, const float* ax1, int64_t n1,
                                             const float* ax2, int64_t n2, int n_shards, const int* devices,
                                             int gather_device, float* d_full, int mode) {
    if (!p || !d_full) return fail(-1, "sdfk_eval_grid_sharded_device: null argument");
    const int n_dev = sdfk_device_count();                      // (none: for_each_shard says so)
    if (n_dev > 0 && (gather_device < 0 || gather_device >= n_dev))
        return fail(-1, "sdfk_eval_grid_sharded_device: gather device out of range");
    return for_each_shard("sdfk_eval_grid_sharded_device", ax0, n0, ax1, n1, ax2, n2, n_shards, devices,
                          [=](int dev, int64_t start, int64_t count) -> int {
        HIPCHK(hipSetDevice(dev));
        hipStream_t stream = nullptr;
        HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        // (SDFK_FORCE_PEER_COPY=1: the copy path also for the shards of the gather device — how a one-GPU box tests it)
        static const bool force_copy = [] { const char* e = getenv("SDFK_FORCE_PEER_COPY"); return e && e[0] == '1'; }();
        const bool in_place = dev == gather_device && !force_copy;
        float* d_slab = in_place ? d_full + start : nullptr;
        int r = 0;
        if (!d_slab && hipMalloc(&d_slab, (size_t)count * sizeof(float)) != hipSuccess) r = fail(-5, "out of device memory for the slab");
        if (r == 0) r = sdfk_eval_grid(p, ax0, n0, ax1, n1, ax2, n2, start, count, d_slab, stream, mode);   // (synchronises)
        if (r == 0 && !in_place) {
            if (hipMemcpyPeerAsync(d_full + start, gather_device, d_slab, dev, (size_t)count * sizeof(float), stream) != hipSuccess ||
                hipStreamSynchronize(stream) != hipSuccess)
                r = fail(-6, "peer copy of the slab failed");
        }
        if (!in_place && d_slab) (void)hipFree(d_slab);
        (void)hipStreamDestroy(stream);
        return r;
    });
}

extern "C" int sdfk_grid_fill(float* d_co, int64_t row_stride, const float* ax0, int64_t n0, const float* ax1,
                              int64_t n1, const float* ax2, int64_t n2, int64_t start, int64_t count, void* stream) {
    if (!d_co) return fail(-1, "sdfk_grid_fill: null output");
    if (row_stride < count) return fail(-1, "sdfk_grid_fill: row stride smaller than count");
    if (start < 0 || count < 0 || start + count > n0 * n1 * n2) return fail(-1, "sdfk_grid_fill: range outside the grid");
    if (count == 0) return 0;
    AxisTables t;
    SrcGrid g;
    int rc = upload_axes(ax0, n0, ax1, n1, ax2, n2, (hipStream_t)stream, &t, &g, start);
    if (rc) return rc;
    hipLaunchKernelGGL(sdfk_gridfill_kernel, dim3(blocks_for(count, 4)), dim3(SDFK_BLOCK), 0, (hipStream_t)stream, g,
                       (long long)count, d_co, (long long)row_stride);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

// ---- host-buffer convenience --------------------------------------------------------------------
// Row length of a host (3, n) array that looks like a flattened meshgrid: the index at which x or y first
// changes (3-D grids: rows along z) or, failing that, at which x first changes (2-D grids: rows along y).
// Only a layout hint for the row-block kernel — a wrong guess costs speed, never correctness.
template <typename T>
static int64_t detect_row_len(const T* co, int64_t n, int64_t stride, bool* flat, int64_t* plane_rows) {
    const int64_t scan = std::min<int64_t>(n, (int64_t)1 << 22);
    const T *x = co, *y = co + stride, *z = co + 2 * stride;
    int64_t a = 0, b = 0;
    *flat = false;
    *plane_rows = 0;
    for (int64_t i = 1; i < scan && (!a || !b); ++i) {
        if (!b && x[i] != x[0]) b = i;
        if (!a && (x[i] != x[0] || y[i] != y[0])) a = i;
    }
    if (a >= 32 && n % a == 0) {
        if (b > a && b % a == 0) *plane_rows = b / a;            // x first changes after b / a rows: one grid plane
        return a;
    }
    if (b >= 32 && n % b == 0) {
        *flat = z[0] == (T)0 && z[b - 1] == (T)0 && z[n - 1] == (T)0;   // (a hint: the kernel checks every point it reads)
        return b;
    }
    return 0;
}

// ---- host arrays in, host array out: a two-slot pipeline over pinned staging buffers ------------------------------
// A pageable (3, n) array cannot be DMA'd directly: hipMemcpy stages it through an internal bounce buffer, one
// synchronous chunk at a time (measured 24-26 GB/s over a 63 GB/s link, kernel and copies never overlapping). Here the
// array is cut into chunks; a few host threads copy (or narrow float64 -> float32) chunk i + 1 into pinned slot B and
// copy chunk i - 1's field out of it, while slot A's stream runs H2D -> kernel -> D2H of chunk i. The pinned slots
// and their device buffers are allocated once per device and kept (256 MiB pinned for 8 Mi-point chunks).
struct HostSlot {
    float *h_co = nullptr, *h_out = nullptr, *d_co = nullptr, *d_out = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    int64_t pending_start = -1, pending_count = 0;        // field in h_out still to be handed to the caller
};
struct HostStage {
    std::mutex mu;                                          // one host-path call per device at a time
    int64_t chunk = 0;
    HostSlot slot[2];
};
static std::mutex g_stage_mu;
static std::map<int, std::unique_ptr<HostStage>> g_stage;
static int host_threads() {
    static int v = [] {
        const char* e = getenv("SDFK_HOST_THREADS");
        int t = e ? atoi(e) : 0;
        if (t < 1) t = std::min(8, std::max(1, (int)std::thread::hardware_concurrency() / 4));
        return std::min(t, 64);
    }();
    return v;
}
// run fn(lo, hi) over [0, count) on the calling thread plus helpers
template <typename F>
static void parallel_ranges(int64_t count, F fn) {
    const int t = (int)std::min<int64_t>(host_threads(), std::max<int64_t>(1, count >> 18));
    if (t <= 1) {
        fn(0, count);
        return;
    }
    std::vector<std::thread> helpers;
    const int64_t step = (count + t - 1) / t;
    for (int i = 1; i < t; ++i) helpers.emplace_back([=] { fn(std::min(count, i * step), std::min(count, (i + 1) * step)); });
    fn(0, std::min(count, step));
    for (std::thread& h : helpers) h.join();
}
static HostStage* stage_of(int device) {
    std::lock_guard<std::mutex> lk(g_stage_mu);
    std::unique_ptr<HostStage>& st = g_stage[device];
    if (!st) st.reset(new HostStage);
    return st.get();
}
// the caller holds st->mu: no other call of this device has anything in flight in the slots being replaced
static int stage_grow(HostStage* st, int64_t want) {
    if (st->chunk >= want) return 0;
    for (HostSlot& sl : st->slot) {
        if (sl.stream) HIPCHK(hipStreamSynchronize(sl.stream));
        if (sl.h_co) (void)hipHostFree(sl.h_co);
        if (sl.h_out) (void)hipHostFree(sl.h_out);
        if (sl.d_co) (void)hipFree(sl.d_co);
        if (sl.d_out) (void)hipFree(sl.d_out);
        sl.h_co = sl.h_out = sl.d_co = sl.d_out = nullptr;
        if (!sl.stream) HIPCHK(hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));
        if (!sl.done) HIPCHK(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
        st->chunk = 0;
        HIPCHK(hipHostMalloc((void**)&sl.h_co, (size_t)want * 3 * sizeof(float), hipHostMallocDefault));
        HIPCHK(hipHostMalloc((void**)&sl.h_out, (size_t)want * sizeof(float), hipHostMallocDefault));
        HIPCHK(hipMalloc(&sl.d_co, (size_t)want * 3 * sizeof(float)));
        HIPCHK(hipMalloc(&sl.d_out, (size_t)want * sizeof(float)));
    }
    st->chunk = want;
    return 0;
}

// out_on_device: `out` is device memory of the same device (the field stays resident, nothing comes back)
static int eval_host_impl(sdfk_program* p, const void* co, int co_dtype, int64_t n, int64_t row_stride, float* out,
                          int device, int mode, bool out_on_device) {
    if (!p) return fail(-1, "null program");
    if (n < 0 || (n > 0 && (!co || !out))) return fail(-1, "sdfk_eval_host: bad arguments");
    if (co_dtype != 0 && co_dtype != 1) return fail(-1, "sdfk_eval_host: co_dtype must be 0 (fp32) or 1 (fp64)");
    if (row_stride < n) return fail(-1, "sdfk_eval_host: row stride smaller than the point count");
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(device));
    static const int64_t max_chunk = [] {
        const char* e = getenv("SDFK_HOST_CHUNK");
        const int64_t v = e ? atoll(e) : 0;
        return v >= 4096 ? v : ((int64_t)1 << 23);           // 8 Mi points: 96 MiB in + 32 MiB out per slot
    }();
    int64_t chunk = std::min<int64_t>(n, max_chunk);
    bool flat = false;
    int64_t plane_rows = 0;
    // SDFK_HOST_TRACE=1: where the call's time goes (stderr, one line per call)
    static const bool trace = [] { const char* e = getenv("SDFK_HOST_TRACE"); return e && e[0] == '1'; }();
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
    const clk::time_point t_call = clk::now();
    double t_stage_in = 0.0, t_wait = 0.0, t_copy_out = 0.0, t_enqueue = 0.0;
    const int64_t row_len = p->sites.empty() ? 0
                            : co_dtype == 0 ? detect_row_len(static_cast<const float*>(co), n, row_stride, &flat, &plane_rows)
                                            : detect_row_len(static_cast<const double*>(co), n, row_stride, &flat, &plane_rows);
    if (row_len > 0 && chunk > row_len) chunk = chunk / row_len * row_len;   // whole rows per chunk
    const int64_t stride = (chunk + 63) & ~(int64_t)63;
    HostStage* st = stage_of(device);
    std::lock_guard<std::mutex> lk(st->mu);                  // one host-path call per device at a time, growth included
    int rc = stage_grow(st, stride);
    if (rc) return rc;
    // the first call of a program builds its kernel: do that before anything is in flight (the build may take seconds)
    auto hand_over = [&](HostSlot& sl) -> int {             // wait for the slot's chunk and give its field to the caller
        if (sl.pending_start < 0) return 0;
        clk::time_point t0 = clk::now();
        HIPCHK(hipEventSynchronize(sl.done));
        t_wait += ms_since(t0);
        if (!out_on_device) {
            t0 = clk::now();
            const float* src = sl.h_out;
            float* dst = out + sl.pending_start;
            parallel_ranges(sl.pending_count, [=](int64_t lo, int64_t hi) { memcpy(dst + lo, src + lo, (size_t)(hi - lo) * sizeof(float)); });
            t_copy_out += ms_since(t0);
        }
        sl.pending_start = -1;
        return 0;
    };
    int k = 0;
    for (int64_t s = 0; s < n && rc == 0; s += chunk, ++k) {
        HostSlot& sl = st->slot[k & 1];
        rc = hand_over(sl);                                  // the slot's previous chunk (two chunks ago) is done: reuse it
        if (rc) break;
        const int64_t m = std::min(chunk, n - s);
        float* h = sl.h_co;
        const clk::time_point t_in = clk::now();
        if (co_dtype == 0) {
            const float* base = static_cast<const float*>(co) + s;
            parallel_ranges(m, [=](int64_t lo, int64_t hi) {
                for (int r = 0; r < 3; ++r) memcpy(h + r * stride + lo, base + r * row_stride + lo, (size_t)(hi - lo) * sizeof(float));
            });
        } else {
            const double* base = static_cast<const double*>(co) + s;
            parallel_ranges(m, [=](int64_t lo, int64_t hi) {
                for (int r = 0; r < 3; ++r) {
                    const double* src = base + r * row_stride;
                    float* dst = h + r * stride;
                    for (int64_t i = lo; i < hi; ++i) dst[i] = (float)src[i];
                }
            });
        }
        t_stage_in += ms_since(t_in);
        const clk::time_point t_enq = clk::now();
        for (int r = 0; r < 3 && rc == 0; ++r)
            if (hipMemcpyAsync(sl.d_co + r * stride, h + r * stride, (size_t)m * sizeof(float), hipMemcpyHostToDevice, sl.stream) != hipSuccess)
                rc = fail(-6, "sdfk_eval_host: host-to-device copy failed");
        if (rc == 0)
            rc = !(row_len > 0 && m % row_len == 0) ? sdfk_eval_device(p, sl.d_co, m, stride, sl.d_out, sl.stream, mode)
                 : flat                             ? sdfk_eval_device_rows2d(p, sl.d_co, m, stride, row_len, sl.d_out, sl.stream, mode)
                 : sdfk_eval_device_rows3d(p, sl.d_co, m, stride, row_len, plane_rows,
                                           plane_rows > 0 ? (s / row_len) % plane_rows : 0, sl.d_out, sl.stream, mode);
        if (rc == 0) {
            const hipError_t e = out_on_device
                                     ? hipMemcpyAsync(out + s, sl.d_out, (size_t)m * sizeof(float), hipMemcpyDeviceToDevice, sl.stream)
                                     : hipMemcpyAsync(sl.h_out, sl.d_out, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, sl.stream);
            if (e != hipSuccess) rc = fail(-6, "sdfk_eval_host: copy of the result failed");
        }
        if (rc == 0 && hipEventRecord(sl.done, sl.stream) != hipSuccess) rc = fail(-6, "sdfk_eval_host: event record failed");
        if (rc == 0) {
            sl.pending_start = s;
            sl.pending_count = m;
        }
        t_enqueue += ms_since(t_enq);
    }
    for (HostSlot& sl : st->slot) {                         // drain (also on errors: nothing of this call stays in flight)
        if (rc == 0) rc = hand_over(sl);
        else {
            (void)hipStreamSynchronize(sl.stream);
            sl.pending_start = -1;
        }
    }
    if (trace)
        fprintf(stderr, "[sdfk host] %lld points, %d chunks of %lld: total %.2f ms = stage-in %.2f + enqueue %.2f + wait %.2f + copy-out %.2f (+ %.2f other)\n",
                (long long)n, k, (long long)chunk, ms_since(t_call), t_stage_in, t_enqueue, t_wait, t_copy_out,
                ms_since(t_call) - t_stage_in - t_enqueue - t_wait - t_copy_out);
    return rc;
}

extern "C" int sdfk_eval_host(sdfk_program* p, const void* co, int co_dtype, int64_t n, int64_t row_stride, float* out,
                              int device, int mode) {
    return eval_host_impl(p, co, co_dtype, n, row_stride, out, device, mode, false);
}
extern "C" int sdfk_eval_host_resident(sdfk_program* p, const void* co, int co_dtype, int64_t n, int64_t row_stride,
                                       float* d_out, int device, int mode) {
    return eval_host_impl(p, co, co_dtype, n, row_stride, d_out, device, mode, true);
}

// ---- plumbing -----------------------------------------------------------------------------------
extern "C" int sdfk_set_device(int device) {
    HIPCHK(hipSetDevice(device));
    return 0;
}
extern "C" void* sdfk_malloc(size_t bytes) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
    if (e != hipSuccess) {
        fail(-5, std::string("hipMalloc: ") + hipGetErrorString(e));
        return nullptr;
    }
    return p;
}
extern "C" int sdfk_free(void* d_ptr) {
    HIPCHK(hipFree(d_ptr));
    return 0;
}
extern "C" int sdfk_memcpy_h2d(void* d_dst, const void* src, size_t bytes) {
    HIPCHK(hipMemcpy(d_dst, src, bytes, hipMemcpyHostToDevice));
    return 0;
}
extern "C" int sdfk_memcpy_d2h(void* dst, const void* d_src, size_t bytes) {
    HIPCHK(hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int sdfk_memcpy_d2d(void* d_dst, const void* d_src, size_t bytes) {
    HIPCHK(hipMemcpy(d_dst, d_src, bytes, hipMemcpyDeviceToDevice));
    return 0;
}
extern "C" int sdfk_sync(void* stream) {
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}
extern "C" void* sdfk_event_create(void) {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) {
        fail(-7, "hipEventCreate failed");
        return nullptr;
    }
    return e;
}
extern "C" int sdfk_event_destroy(void* ev) {
    HIPCHK(hipEventDestroy((hipEvent_t)ev));
    return 0;
}
extern "C" int sdfk_event_record(void* ev, void* stream) {
    HIPCHK(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream));
    return 0;
}
extern "C" int sdfk_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms) {
    HIPCHK(hipEventSynchronize((hipEvent_t)ev_stop));
    HIPCHK(hipEventElapsedTime(ms, (hipEvent_t)ev_start, (hipEvent_t)ev_stop));
    return 0;
}
extern "C" int sdfk_stream_probe(const float* d_co, int64_t n, int64_t row_stride, float* d_out, void* stream) {
    if (!d_co || !d_out) return fail(-1, "sdfk_stream_probe: null pointer");
    if (!(aligned16(d_co) && aligned16(d_out) && row_stride % 4 == 0 && n % 4 == 0))
        return fail(-1, "sdfk_stream_probe: needs 16-byte aligned rows and n % 4 == 0");
    SrcArray a = {d_co, (long long)row_stride};
    hipLaunchKernelGGL(sdfk_probe_kernel, dim3(blocks_for(n, 4)), dim3(SDFK_BLOCK), 0, (hipStream_t)stream, a,
                       (long long)n, d_out);
    HIPCHK(hipGetLastError());
    return 0;
}

#include "sdfk_gridops.inc"
#include "sdfk_fieldops.inc"
#include "sdfk_vector.inc"
#include "sdfk_hosttree.inc"
#include "sdfk_lcwg.inc"
#include "sdfk_dual.inc"
#include "sdfk_project.inc"
#include "sdfk_adjoint.inc"
#include "sdfk_points.inc"
#include "sdfk_mesh.inc"
#include "sdfk_slices.inc"
#include "sdfk_topology.inc"
#include "sdfk_layers.inc"
#include "sdfk_rays.inc"
#include "sdfk_occupancy.inc"
#include "sdfk_moments.inc"
#include "sdfk_redistance.inc"
#include "sdfk_enclosure.inc"
