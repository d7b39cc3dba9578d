// sdfk_occupancy.inc — sub-voxel occupancy of a program on a grid: per cell, the fraction of its k^d sub-sample points
// that lie in the solid (included at the end of sdfk.hip, after sdfk_rays.inc; the sample pass itself: sdfk_occdev.h; the
// definition for users: aegolius_amd/occupancy.py). The host side of the sub-sample lattice is here once, for this entry
// and for sdfk_eval_grid_moments (sdfk_moments.inc): occ_request checks a call's arguments, occ_open uploads the tables,
// occ_tail lays out the scratch both share, and occ_slabs drives the passes, handing a consumer the two steps that differ
// — the second classify pass and the sample pass. Slabs of whole rows, three passes per slab (as occupancy runs them):
//
//   1. centre values : run() — the grid evaluation of sdfk_eval_grid, every fast kernel unchanged — writes f at the grid
//      points of the slab into 4 B per cell of scratch.
//   2. classify      : a cell is FAR iff
//          |f(c) - level| > 1.0001 L rho + L cmag + 1e-6 (1 + |f(c)| + |level|),  cmag = 1e-6 (|cx| + |cy| + |cz| + rho),
//      rho = sqrt(hw0^2 + hw1^2 + hw2^2) the distance from c to the farthest sub-sample (half-width tables, rounded up on
//      the host), L the Lipschitz bound of the field: then no sub-sample can lie on the other side of the level, and the
//      cell gets 1.0 / 0.0 by its centre. The comparison is false for a NaN on either side (tested on the bits: the
//      kernels are built with -fno-honor-nans), so such a cell is NEAR. The near cells' slab-relative indices are
//      compacted into a list, in ascending order, without atomics: sdfk_occ_classify_kernel<false> counts the near cells of every
//      wave's run of 1024 consecutive cells, the selection's scan (sdfk_select_scan_kernel) turns the counts into offsets,
//      and sdfk_occ_classify_kernel<true> decides again (the same function of the same inputs), stores 0.0 / 1.0 for the far
//      cells and the near cells' indices at offset + rank (one ballot per round). One vector atomic per wave on a list
//      head was the first version: with every wave of the device on one address it cost 11 ns per wave, more than the rest
//      of the pass (DESIGN 4.15 has the numbers).
//   3. sample        : sdfk_occ_sample over the list — the interpreter kernel below or the specialised flavour
//      (SDFK_FL_OCCUPANCY), same text, same bits.
// Without a finite bound, and under SDFK_MODE_NOCULL, passes 1 and 2 are left out and pass 3 takes every cell.
// Every output element is written exactly once, by pass 2 or pass 3, with plain vector stores. After the last slab
// sdfk_occ_total_kernel adds up fraction * K — integers — over the whole output: per-wave partial sums in a fixed order,
// added on the host. Scratch: 32 KB (those partial sums), then the lattice's tail (occ_tail): 8 B per 1024 slab cells
// (counts) and 8 B per slab cell (centre values, list).
#include "sdfk_interpfield.h"
#include "sdfk_occdev.h"

template <int NC, int NV, typename SRC>
__global__ __launch_bounds__(SDFK_OCC_BLOCK) void sdfk_occ_interp_kernel(const uint2* __restrict__ code, int n_instr,
                                                                        const float* __restrict__ prm,
                                                                        const float* __restrict__ tab, int result_reg, SRC src,
                                                                        sdfk_occgrid grid, float* __restrict__ out) {
    const SdfkInterpField<NC, NV> field = {code, n_instr, prm, tab, result_reg};
    sdfk_occ_sample(src, field, grid, out);
}

#define SDFK_OCC_RUN 1024              // consecutive cells one wave of the classify kernels owns: 16 rounds of 64
#define SDFK_OCC_PARTIALS 4096         // waves of the total kernel

struct sdfk_occclass {
    const float* __restrict__ ax0;     // the caller's axis tables (what pass 1 read) and the half-widths, per axis
    const float* __restrict__ ax1;
    const float* __restrict__ ax2;
    const float* __restrict__ hw0;
    const float* __restrict__ hw1;
    const float* __restrict__ hw2;
    unsigned n1, n2;
    long long first, count;            // the slab: flat index of its cell 0, its cells
    float level, lip;
    unsigned level_key;
};
static __device__ __forceinline__ bool sdfk_occ_number(float v) {
    return (__builtin_bit_cast(unsigned, v) & 0x7fffffffu) <= 0x7f800000u;
}
// Walks a wave's run of cells 64 at a time: (ix0, iy0, iz0) are the indices of lane 0's cell (wave-uniform; the 64-bit
// divisions happen once per wave, on the scalar unit), the lanes add their offset in 32 bits, as sdfk_load(SrcGrid) does.
struct SdfkOccWalk {
    unsigned long long ix0;
    unsigned iy0, iz0;
    __device__ __forceinline__ void start(unsigned long long flat, unsigned n1, unsigned n2) {
        const unsigned long long row = flat / n2;
        iz0 = (unsigned)(flat - row * n2);
        ix0 = row / n1;
        iy0 = (unsigned)(row - ix0 * n1);
    }
    __device__ __forceinline__ void lane(unsigned l, unsigned n1, unsigned n2, unsigned long long& i0, unsigned& i1,
                                         unsigned& i2) const {
        const unsigned t = iz0 + l, cz = t / n2, ty = iy0 + cz, cy = ty / n1;
        i2 = t - cz * n2;
        i1 = ty - cy * n1;
        i0 = ix0 + cy;
    }
    __device__ __forceinline__ void advance(unsigned n1, unsigned n2) {   // 64 cells on
        const unsigned t = iz0 + 64u, cz = t / n2, ty = iy0 + cz, cy = ty / n1;
        iz0 = t - cz * n2;
        iy0 = ty - cy * n1;
        ix0 += cy;
    }
};
// -> is the cell near; *inside = f <= level
static __device__ __forceinline__ bool sdfk_occ_near(const sdfk_occclass& C, float f, unsigned long long i0, unsigned i1,
                                                     unsigned i2, bool* inside) {
    const float h0 = C.hw0[i0], h1 = C.hw1[i1], h2 = C.hw2[i2];
    const float rho = sqrtf(fmaf(h2, h2, fmaf(h1, h1, h0 * h0)));
    const float cmag = 1e-6f * (fabsf(C.ax0[i0]) + fabsf(C.ax1[i1]) + fabsf(C.ax2[i2]) + rho);
    const float rhs = ((1.0001f * C.lip) * rho + C.lip * cmag) + 1e-6f * ((1.0f + fabsf(f)) + fabsf(C.level));
    const float lhs = fabsf(f - C.level);
    *inside = sdfk_sel_key(f) <= C.level_key;
    return !(sdfk_occ_number(lhs) && sdfk_occ_number(rhs) && lhs > rhs);
}
// WRITE = false: blk[wave] = near cells of the wave's run. WRITE = true: blk holds the exclusive offsets; far cells get
// 0.0 / 1.0, near cells go to the list.
template <bool WRITE>
__global__ __launch_bounds__(SDFK_OCC_BLOCK) void sdfk_occ_classify_kernel(const float* __restrict__ centre, sdfk_occclass C,
                                                                          float* __restrict__ out, unsigned* __restrict__ list,
                                                                          unsigned long long* __restrict__ blk) {
    const unsigned lane = sdfk_tx() & 63u;
    const long long wave = (long long)sdfk_bx() * (SDFK_OCC_BLOCK / 64) + (sdfk_tx() >> 6);
    const long long begin = wave * SDFK_OCC_RUN;
    if (begin >= C.count) return;                               // (wave-uniform)
    SdfkOccWalk walk;
    walk.start((unsigned long long)(C.first + begin), C.n1, C.n2);
    unsigned long long at = WRITE ? blk[wave] : 0ull;
    for (int r = 0; r < SDFK_OCC_RUN / 64; ++r) {
        const long long i = begin + r * 64 + lane;
        const bool active = i < C.count;
        bool near_cell = false, inside = false;
        if (active) {
            unsigned long long i0;
            unsigned i1, i2;
            walk.lane(lane, C.n1, C.n2, i0, i1, i2);
            near_cell = sdfk_occ_near(C, centre[i], i0, i1, i2, &inside);
        }
        const unsigned long long nb = __ballot(near_cell);
        if constexpr (WRITE) {
            const unsigned long long slot = at + (unsigned)__popcll(nb & ((1ull << lane) - 1ull));
            if (near_cell && slot < (unsigned long long)C.count) list[slot] = (unsigned)i;
            else if (active && !near_cell) out[i] = inside ? 1.0f : 0.0f;
        }
        at += (unsigned)__popcll(nb);
        walk.advance(C.n1, C.n2);
    }
    if (!WRITE && lane == 0u) blk[wave] = at;
}

// partial[w] = sum over the cells of wave w of fraction * K (integers: the counts), grid-stride in a fixed order
__global__ __launch_bounds__(256) void sdfk_occ_total_kernel(const float* __restrict__ out, long long n, float K,
                                                             unsigned long long* __restrict__ partial) {
    const unsigned lane = sdfk_tx() & 63u;
    const long long wave = (long long)sdfk_bx() * 4 + (sdfk_tx() >> 6);
    unsigned long long sum = 0;
    for (long long i = wave * 64 + lane; i < n; i += (long long)SDFK_OCC_PARTIALS * 64) sum += (unsigned)(out[i] * K);
    unsigned lo = (unsigned)sum, hi = (unsigned)(sum >> 32);
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long other = ((unsigned long long)__shfl_down(hi, off) << 32) | __shfl_down(lo, off);
        sum += other;
        lo = (unsigned)sum;
        hi = (unsigned)(sum >> 32);
    }
    if (lane == 0u) partial[wave] = sum;
}

// S[r] = sum over i of field[r row_len + i] * weight[i], in float64, one wave per row: lane l adds i = l, l + 64, ... in that
// order and the 64 partial sums are folded by halves — a fixed order, so the sums do not vary between runs.
__global__ __launch_bounds__(256) void sdfk_row_sums_kernel(const float* __restrict__ field, long long rows, long long row_len,
                                                            const double* __restrict__ weight, double* __restrict__ out) {
    const long long r = (long long)sdfk_bx() * 4 + (sdfk_tx() >> 6);
    if (r >= rows) return;                                     // (wave-uniform)
    const unsigned lane = sdfk_tx() & 63u;
    const float* __restrict__ line = field + r * row_len;
    double sum = 0.0;
    for (long long i = lane; i < row_len; i += 64) sum += (double)line[i] * weight[i];
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
    if (lane == 0u) out[r] = sum;
}

// ---- host side ----------------------------------------------------------------------------------
extern "C" int sdfk_field_row_sums(const float* d_field, int64_t rows, int64_t row_len, const double* weights, double* d_out,
                                   void* stream_) {
    if (rows < 0 || row_len < 0) return fail(-1, "sdfk_field_row_sums: negative size");
    if (rows == 0) return 0;
    if (!d_field || !d_out || (row_len > 0 && !weights)) return fail(-1, "sdfk_field_row_sums: null pointer");
    if ((rows + 3) / 4 > 0x7fffffffLL) return fail(-1, "sdfk_field_row_sums: too many rows");
    hipStream_t stream = (hipStream_t)stream_;
    struct Weights {
        double* d = nullptr;
        ~Weights() { if (d) (void)hipFree(d); }
    } w;
    HIPCHK(hipMalloc(&w.d, (size_t)std::max<int64_t>(row_len, 1) * sizeof(double)));
    HIPCHK(hipMemcpyAsync(w.d, weights, (size_t)row_len * sizeof(double), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(sdfk_row_sums_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, d_field, (long long)rows,
                       (long long)row_len, (const double*)w.d, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(stream));                       // the weights are freed on return
    return 0;
}

static constexpr int64_t kOccSlabDefault = 1LL << 30;
// cells of one slab: whole rows (along the last axis that is longer than one point), at most slab_cells unless one row is longer
static int64_t occ_slab_cells(int64_t n0, int64_t n1, int64_t n2, int64_t slab_cells) {
    const int64_t total = n0 * n1 * n2;
    const int64_t row = n2 > 1 ? n2 : n1;
    if (slab_cells <= 0) slab_cells = kOccSlabDefault;
    slab_cells = std::min(slab_cells, kOccSlabDefault);
    const int64_t rows = std::max<int64_t>(1, slab_cells / std::max<int64_t>(row, 1));
    return std::min(total, rows * row);
}
// (bit tests: this file is built with -fno-honor-nans, which leaves isnan / isfinite of a NaN undefined on the host too)
static unsigned occ_bits(float v) {
    unsigned u;
    memcpy(&u, &v, sizeof u);
    return u & 0x7fffffffu;
}
static bool occ_is_nan(float v) { return occ_bits(v) > 0x7f800000u; }
static bool occ_is_finite(float v) { return occ_bits(v) < 0x7f800000u; }
static size_t occ_align(size_t bytes) { return (bytes + 255) / 256 * 256; }
static int64_t occ_runs(int64_t cells) { return (cells + SDFK_OCC_RUN - 1) / SDFK_OCC_RUN; }

// ---- the lattice: what every consumer of the sub-samples shares (sdfk_eval_grid_occupancy, sdfk_eval_grid_moments) ----
// A call: the entry's arguments as it got them (the tables are host pointers nobody has read), then what occ_request adds.
struct OccRequest {
    sdfk_program* p;
    const float* ax[3];
    const float* sub[3];
    const float* hw[3];
    int64_t n[3];
    int samples;
    float level, lipschitz;
    int64_t slab_cells;
    int mode;                          // (occ_request resolves SDFK_MODE_AUTO)
    unsigned k[3], lg[3], K;           // sub-samples per axis (1 on an axis of one point), their log2s, k0 k1 k2
    unsigned per_wave;                 // entries of one wave of the sample kernels (sdfk_occdev.h, sdfk_momdev.h)
    bool skip;                         // passes 1 and 2 run: far cells are settled by their centre
    int64_t total_cells, slab;
};
// The checks both entries make, in `w`'s name, and the derived fields; n0_max: the longest axis 0 the entry takes.
static int occ_request(const std::string& w, int64_t n0_max, OccRequest* q) {
    if (!q->p) return fail(-1, "null program");
    for (int a = 0; a < 3; ++a)
        if (!q->ax[a] || !q->sub[a] || !q->hw[a]) return fail(-1, w + ": null table");
    const int64_t* n = q->n;
    if (n[0] < 1 || n[1] < 1 || n[2] < 1 || n[1] > 0x7fffffff || n[2] > 0x7fffffff || n[0] > n0_max)
        return fail(-1, w + ": axis sizes from 1 to 2^31 - 1");
    const int k = q->samples;
    if (k != 1 && k != 2 && k != 4 && k != 8) return fail(-1, w + ": samples per axis: 1, 2, 4 or 8");
    if (occ_is_nan(q->level)) return fail(-1, w + ": the level is NaN");
    if (occ_is_nan(q->lipschitz) || q->lipschitz < 0.0f) return fail(-1, w + ": the Lipschitz bound must not be negative or NaN");
    if (q->mode < SDFK_MODE_AUTO || q->mode > SDFK_MODE_NOCULL) return fail(-1, w + ": unknown mode");
    int bad = -1;
    const int chk = sdfk_program_rays_check(q->p, &bad);
    if (chk) return fail(chk < 0 ? chk : -3, w + ": " + g_err);
    if (q->mode == SDFK_MODE_AUTO) q->mode = g_default_mode;
    q->skip = occ_is_finite(q->lipschitz) && q->mode != SDFK_MODE_NOCULL;
    q->K = 1;
    for (int a = 0; a < 3; ++a) {
        q->k[a] = n[a] > 1 ? (unsigned)k : 1u;
        q->lg[a] = q->k[a] == 8 ? 3u : q->k[a] == 4 ? 2u : q->k[a] == 2 ? 1u : 0u;
        q->K *= q->k[a];
    }
    q->per_wave = q->K >= 64u ? 1u : 64u / q->K;
    q->total_cells = n[0] * n[1] * n[2];
    q->slab = occ_slab_cells(n[0], n[1], n[2], q->slab_cells);
    return 0;
}

// What a call holds on the device until it returns: the program, the sample pass's kernel (the same for every slab; null:
// the interpreter kernel), the tables, and the two structs the kernels take, whose slab fields occ_slabs sets.
struct OccTables {
    LaunchCtx x;
    std::shared_ptr<SpecModule> sk;
    AxisTables axes, extra;            // the axis tables as sdfk_eval_grid uploads them | the sub-sample tables, the half-widths
    SrcGrid g;
    sdfk_occgrid G;
    sdfk_occclass C;
};
// flavour, what: the sample kernel's (a failed build falls back in AUTO only)
static int occ_open(const OccRequest& q, void* stream_, int flavour, const char* what, OccTables* t) {
    int rc = launch_ctx(q.p, stream_, &t->x);
    if (rc) return rc;
    hipStream_t stream = t->x.stream;
    rc = pick_kernel(q.p, t->x.device, flavour, 0, q.mode, q.mode == SDFK_MODE_AUTO, what, false, &t->sk);
    if (rc) return rc;
    const int64_t* n = q.n;
    rc = upload_axes(q.ax[0], n[0], q.ax[1], n[1], q.ax[2], n[2], stream, &t->axes, &t->g, 0);
    if (rc) return rc;
    const size_t s0 = (size_t)n[0] * q.k[0], s1 = (size_t)n[1] * q.k[1], s2 = (size_t)n[2] * q.k[2];
    HIPCHK(hipMalloc(&t->extra.d, (s0 + s1 + s2 + (size_t)(n[0] + n[1] + n[2])) * sizeof(float)));
    float* d_sub[3] = {t->extra.d, t->extra.d + s0, t->extra.d + s0 + s1};
    float* d_hw[3] = {d_sub[2] + s2, d_sub[2] + s2 + n[0], d_sub[2] + s2 + n[0] + n[1]};
    for (int a = 0; a < 3; ++a)
        HIPCHK(hipMemcpyAsync(d_sub[a], q.sub[a], (size_t)n[a] * q.k[a] * sizeof(float), hipMemcpyHostToDevice, stream));
    for (int a = 0; a < 3; ++a) HIPCHK(hipMemcpyAsync(d_hw[a], q.hw[a], (size_t)n[a] * sizeof(float), hipMemcpyHostToDevice, stream));
    sdfk_occgrid G = {d_sub[0], d_sub[1], d_sub[2], (unsigned)n[1], (unsigned)n[2], q.k[1], q.k[2], q.k[0], q.lg[1], q.lg[2], q.K,
                      q.lg[0] + q.lg[1] + q.lg[2], 1.0f / (float)q.K, sdfk_sel_key(q.level), q.total_cells < (1LL << 32) ? 1u : 0u, 0};
    sdfk_occclass C = {t->g.ax0, t->g.ax1, t->g.ax2, d_hw[0], d_hw[1], d_hw[2], (unsigned)n[1], (unsigned)n[2], 0, 0, q.level,
                       q.lipschitz, sdfk_sel_key(q.level)};
    t->G = G, t->C = C;
    return 0;
}

// The tail of either entry's scratch, after the consumer's own head: (runs + 1) counts / offsets | centre values | list
struct OccTail {
    unsigned long long* d_blk;
    float* d_centre;
    unsigned* d_list;
};
static size_t occ_tail_bytes(int64_t slab) { return occ_align((size_t)(occ_runs(slab) + 1) * 8) + 2 * occ_align((size_t)slab * 4); }
static OccTail occ_tail(char* base, int64_t slab) {
    char* centre = base + occ_align((size_t)(occ_runs(slab) + 1) * 8);
    return {(unsigned long long*)base, (float*)centre, (unsigned*)(centre + occ_align((size_t)slab * 4))};
}

// The sample kernel of a consumer over `src` (SdfkOccList or SdfkOccAll): the specialised flavour's, or the interpreter
// kernel CONSUMER::interp_kernel<NC, NV, SRC>() names. tail: the kernel's arguments after the grid.
template <typename CONSUMER, typename SRC, typename... TAIL>
static int occ_sample_launch(const OccRequest& q, const OccTables& t, SRC src, unsigned blocks, TAIL... tail) {
    const LaunchCtx& x = t.x;
    const float* prm = x.prm;
    const float* tab = x.tab;
    sdfk_occgrid G = t.G;
    if (t.sk) {
        void* args[] = {&prm, &tab, &src, &G, (void*)&tail...};
        HIPCHK(hipModuleLaunchKernel(t.sk->fn[std::is_same_v<SRC, SdfkOccList> ? 0 : 1], blocks, 1, 1, SDFK_OCC_BLOCK, 1, 1, 0,
                                     x.stream, args, nullptr));
    } else {
#define SDFK_OCC_GO(NC, NV) hipLaunchKernelGGL((CONSUMER::template interp_kernel<NC, NV, SRC>()), dim3(blocks), dim3(SDFK_OCC_BLOCK), 0, x.stream, \
                                               x.d->d_code, x.n_instr, prm, tab, x.result_reg, src, G, tail...)
        SDFK_REGFILE(q.p, SDFK_NC, SDFK_NV, SDFK_OCC_GO);
#undef SDFK_OCC_GO
        HIPCHK(hipGetLastError());
    }
    return 0;
}

struct OccEvents {
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    ~OccEvents() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
};

// The loop over the slabs of a call, for the consumer `c`: per slab the centre pass, the count of the near cells of every
// run and its scan, c's own second classify pass, the near count read back, and c's sample pass over the list (or over
// every cell where nothing is skipped). pass_ms, if given, receives the three passes' device-event milliseconds;
// near_cells the cells sampled, after the last slab. c has
//     int classify(t, s, first, runs, blocks)   launch the second classify pass of the slab at `first` (s.d_blk: the offsets)
//     int classified(stream)                    synchronise the stream: the near count is then on the host
//     int sample(q, t, src, first)              launch the sample pass over src's entries
//     int sampled(stream)                       after the sample pass's event: whatever c reads back from it
template <typename CONSUMER>
static int occ_slabs(const std::string& w, const OccRequest& q, OccTables& t, const OccTail& s, float* pass_ms, CONSUMER& c,
                     int64_t* near_cells) {
    hipStream_t stream = t.x.stream;
    OccEvents ev;
    if (pass_ms) {
        for (hipEvent_t& e : ev.e) HIPCHK(hipEventCreate(&e));
        pass_ms[0] = pass_ms[1] = pass_ms[2] = 0.0f;
    }
    int64_t near_total = 0;
    for (int64_t first = 0; first < q.total_cells; first += q.slab) {
        const int64_t cells = std::min(q.slab, q.total_cells - first);
        unsigned long long n_entries = (unsigned long long)cells;
        int rc;
        if (pass_ms) HIPCHK(hipEventRecord(ev.e[0], stream));
        if (q.skip) {
            t.g.start = first;
            rc = run(grid_call(q.p, &t.g, cells, s.d_centre, stream, q.mode, true));
            if (rc) return rc;
            if (pass_ms) HIPCHK(hipEventRecord(ev.e[1], stream));
            t.C.first = first;
            t.C.count = cells;
            const long long runs = occ_runs(cells);
            const unsigned blocks = (unsigned)((runs + SDFK_OCC_BLOCK / 64 - 1) / (SDFK_OCC_BLOCK / 64));
            hipLaunchKernelGGL(sdfk_occ_classify_kernel<false>, dim3(blocks), dim3(SDFK_OCC_BLOCK), 0, stream,
                               (const float*)s.d_centre, t.C, (float*)nullptr, s.d_list, s.d_blk);
            hipLaunchKernelGGL(sdfk_select_scan_kernel, dim3(1), dim3(1024), 0, stream, s.d_blk, runs);
            rc = c.classify(t, s, first, runs, blocks);
            if (rc) return rc;
            HIPCHK(hipGetLastError());
            unsigned long long h = 0;
            HIPCHK(hipMemcpyAsync(&h, s.d_blk + runs, sizeof h, hipMemcpyDeviceToHost, stream));
            rc = c.classified(stream);
            if (rc) return rc;
            if (h > (unsigned long long)cells) return fail(-2, w + ": the list of near cells is longer than the slab");
            n_entries = h;
        } else if (pass_ms) {
            HIPCHK(hipEventRecord(ev.e[1], stream));
        }
        if (pass_ms) HIPCHK(hipEventRecord(ev.e[2], stream));
        near_total += (int64_t)n_entries;
        if (n_entries) {
            t.G.first = first;
            rc = q.skip ? c.sample(q, t, SdfkOccList{s.d_list, n_entries}, first) : c.sample(q, t, SdfkOccAll{n_entries}, first);
            if (rc) return rc;
        }
        if (pass_ms) HIPCHK(hipEventRecord(ev.e[3], stream));
        if (n_entries) {
            rc = c.sampled(stream);
            if (rc) return rc;
        }
        if (pass_ms) {
            HIPCHK(hipEventSynchronize(ev.e[3]));
            for (int k = 0; k < 3; ++k) {
                float ms = 0.0f;
                HIPCHK(hipEventElapsedTime(&ms, ev.e[k], ev.e[k + 1]));
                pass_ms[k] += ms;
            }
        }
    }
    *near_cells = near_total;
    return 0;
}

// ---- occupancy --------------------------------------------------------------------------------------------------------
// scratch layout: the total kernel's partial sums | the lattice's tail
extern "C" size_t sdfk_eval_grid_occupancy_scratch(int64_t n0, int64_t n1, int64_t n2, int64_t slab_cells) {
    if (n0 < 1 || n1 < 1 || n2 < 1) return 0;
    return SDFK_OCC_PARTIALS * 8 + occ_tail_bytes(occ_slab_cells(n0, n1, n2, slab_cells));
}

// occ_slabs' consumer: every cell's fraction, written once by the second classify pass or by the sample pass
struct OccFractions {
    float* d_fraction;
    template <int NC, int NV, typename SRC>
    static auto interp_kernel() { return sdfk_occ_interp_kernel<NC, NV, SRC>; }
    int classify(const OccTables& t, const OccTail& s, int64_t first, long long, unsigned blocks) {
        hipLaunchKernelGGL(sdfk_occ_classify_kernel<true>, dim3(blocks), dim3(SDFK_OCC_BLOCK), 0, t.x.stream,
                           (const float*)s.d_centre, t.C, d_fraction + first, s.d_list, s.d_blk);
        return 0;
    }
    int classified(hipStream_t stream) { HIPCHK(hipStreamSynchronize(stream)); return 0; }
    template <typename SRC>
    int sample(const OccRequest& q, const OccTables& t, SRC src, int64_t first) {
        const unsigned long long waves = (src.n + q.per_wave - 1) / q.per_wave;
        const unsigned blocks = (unsigned)((waves + SDFK_OCC_BLOCK / 64 - 1) / (SDFK_OCC_BLOCK / 64));
        return occ_sample_launch<OccFractions>(q, t, src, blocks, d_fraction + first);
    }
    int sampled(hipStream_t) { return 0; }
};

extern "C" int sdfk_eval_grid_occupancy(sdfk_program* p, const float* ax0, int64_t n0, const float* ax1, int64_t n1,
                                        const float* ax2, int64_t n2, const float* sub0, const float* sub1, const float* sub2,
                                        const float* hw0, const float* hw1, const float* hw2, int samples, float level,
                                        float lipschitz, float* d_fraction, void* d_scratch, int64_t slab_cells,
                                        int64_t* inside_samples, int64_t* near_cells, float* pass_ms, void* stream_, int mode) {
    const std::string w = "sdfk_eval_grid_occupancy";
    OccRequest q = {p, {ax0, ax1, ax2}, {sub0, sub1, sub2}, {hw0, hw1, hw2}, {n0, n1, n2}, samples, level, lipschitz, slab_cells, mode};
    int rc = occ_request(w, 1LL << 40, &q);
    if (rc) return rc;
    if (!d_fraction || !d_scratch) return fail(-1, w + ": null output or scratch pointer");
    if (!inside_samples || !near_cells) return fail(-1, w + ": null statistics pointer");

    OccTables t;
    rc = occ_open(q, stream_, SDFK_FL_OCCUPANCY, "occupancy kernel", &t);
    if (rc) return rc;
    hipStream_t stream = t.x.stream;
    unsigned long long* d_partial = (unsigned long long*)d_scratch;
    OccFractions fractions = {d_fraction};
    rc = occ_slabs(w, q, t, occ_tail((char*)d_scratch + SDFK_OCC_PARTIALS * 8, q.slab), pass_ms, fractions, near_cells);
    if (rc) return rc;
    // the sum of the counts, from the fractions: integers, whatever the order
    hipLaunchKernelGGL(sdfk_occ_total_kernel, dim3(SDFK_OCC_PARTIALS / 4), dim3(256), 0, stream, (const float*)d_fraction,
                       (long long)q.total_cells, (float)q.K, d_partial);
    HIPCHK(hipGetLastError());
    std::vector<unsigned long long> partial(SDFK_OCC_PARTIALS);
    HIPCHK(hipMemcpyAsync(partial.data(), d_partial, partial.size() * 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));                       // the tables are freed on return
    unsigned long long inside = 0;
    for (unsigned long long v : partial) inside += v;
    *inside_samples = (int64_t)inside;
    return 0;
}
