// sdfk_occupancy.inc — sub-voxel occupancy of a program on a grid: per cell, the fraction of its k^d sub-sample points
// that lie in the solid (included at the end of sdfk.hip, after sdfk_rays.inc; the sample pass itself: sdfk_occdev.h; the
// definition for users: aegolius_amd/occupancy.py). Slabs of whole rows, three passes per slab:
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
// added on the host. Scratch: 8 B per slab cell (centre values, list), 8 B per 1024 slab cells (counts) and 32 KB.
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

// scratch layout: the total kernel's partial sums | (runs + 1) counts / offsets | centre values | list
extern "C" size_t sdfk_eval_grid_occupancy_scratch(int64_t n0, int64_t n1, int64_t n2, int64_t slab_cells) {
    if (n0 < 1 || n1 < 1 || n2 < 1) return 0;
    const int64_t slab = occ_slab_cells(n0, n1, n2, slab_cells);
    return SDFK_OCC_PARTIALS * 8 + occ_align((size_t)(occ_runs(slab) + 1) * 8) + 2 * occ_align((size_t)slab * 4);
}

struct OccEvents {
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    ~OccEvents() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
};

extern "C" int sdfk_eval_grid_occupancy(sdfk_program* p, const float* ax0, int64_t n0, const float* ax1, int64_t n1,
                                        const float* ax2, int64_t n2, const float* sub0, const float* sub1, const float* sub2,
                                        const float* hw0, const float* hw1, const float* hw2, int samples, float level,
                                        float lipschitz, float* d_fraction, void* d_scratch, int64_t slab_cells,
                                        int64_t* inside_samples, int64_t* near_cells, float* pass_ms, void* stream_, int mode) {
    const std::string w = "sdfk_eval_grid_occupancy";
    if (!p) return fail(-1, "null program");
    if (!ax0 || !ax1 || !ax2 || !sub0 || !sub1 || !sub2 || !hw0 || !hw1 || !hw2) return fail(-1, w + ": null table");
    if (n0 < 1 || n1 < 1 || n2 < 1 || n1 > 0x7fffffff || n2 > 0x7fffffff || n0 > (1LL << 40))
        return fail(-1, w + ": axis sizes from 1 to 2^31 - 1");
    if (samples != 1 && samples != 2 && samples != 4 && samples != 8) return fail(-1, w + ": samples per axis: 1, 2, 4 or 8");
    if (occ_is_nan(level)) return fail(-1, w + ": the level is NaN");
    if (occ_is_nan(lipschitz) || lipschitz < 0.0f) return fail(-1, w + ": the Lipschitz bound must not be negative or NaN");
    if (!d_fraction || !d_scratch) return fail(-1, w + ": null output or scratch pointer");
    if (!inside_samples || !near_cells) return fail(-1, w + ": null statistics pointer");
    if (mode < SDFK_MODE_AUTO || mode > SDFK_MODE_NOCULL) return fail(-1, w + ": unknown mode");
    int bad = -1;
    const int chk = sdfk_program_rays_check(p, &bad);
    if (chk) return fail(chk < 0 ? chk : -3, w + ": " + g_err);
    if (mode == SDFK_MODE_AUTO) mode = g_default_mode;
    const bool skip = occ_is_finite(lipschitz) && mode != SDFK_MODE_NOCULL;

    const unsigned k0 = n0 > 1 ? samples : 1, k1 = n1 > 1 ? samples : 1, k2 = n2 > 1 ? samples : 1;
    auto lg = [](unsigned k) { return k == 8 ? 3u : k == 4 ? 2u : k == 2 ? 1u : 0u; };
    const unsigned K = k0 * k1 * k2;
    const int64_t total_cells = n0 * n1 * n2;
    const int64_t slab = occ_slab_cells(n0, n1, n2, slab_cells);

    LaunchCtx x;
    int rc = launch_ctx(p, stream_, &x);
    if (rc) return rc;
    hipStream_t stream = x.stream;
    // the sample pass's kernel, the same for every slab (a failed build falls back in AUTO only)
    std::shared_ptr<SpecModule> sk;
    rc = pick_kernel(p, x.device, SDFK_FL_OCCUPANCY, 0, mode, mode == SDFK_MODE_AUTO, "occupancy kernel", false, &sk);
    if (rc) return rc;

    // tables: the axis tables as sdfk_eval_grid uploads them, then the sub-sample tables and the half-widths
    AxisTables axes, extra;
    SrcGrid g;
    rc = upload_axes(ax0, n0, ax1, n1, ax2, n2, stream, &axes, &g, 0);
    if (rc) return rc;
    const size_t s0 = (size_t)n0 * k0, s1 = (size_t)n1 * k1, s2 = (size_t)n2 * k2;
    HIPCHK(hipMalloc(&extra.d, (s0 + s1 + s2 + (size_t)(n0 + n1 + n2)) * sizeof(float)));
    float* d_sub[3] = {extra.d, extra.d + s0, extra.d + s0 + s1};
    float* d_hw[3] = {extra.d + s0 + s1 + s2, extra.d + s0 + s1 + s2 + n0, extra.d + s0 + s1 + s2 + n0 + n1};
    HIPCHK(hipMemcpyAsync(d_sub[0], sub0, s0 * sizeof(float), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_sub[1], sub1, s1 * sizeof(float), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_sub[2], sub2, s2 * sizeof(float), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_hw[0], hw0, (size_t)n0 * sizeof(float), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_hw[1], hw1, (size_t)n1 * sizeof(float), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_hw[2], hw2, (size_t)n2 * sizeof(float), hipMemcpyHostToDevice, stream));

    char* scratch = (char*)d_scratch;
    unsigned long long* d_partial = (unsigned long long*)scratch;
    unsigned long long* d_blk = (unsigned long long*)(scratch + SDFK_OCC_PARTIALS * 8);
    char* rest = scratch + SDFK_OCC_PARTIALS * 8 + occ_align((size_t)(occ_runs(slab) + 1) * 8);
    float* d_centre = (float*)rest;
    unsigned* d_list = (unsigned*)(rest + occ_align((size_t)slab * 4));

    OccEvents ev;
    if (pass_ms) {
        for (hipEvent_t& x : ev.e) HIPCHK(hipEventCreate(&x));
        pass_ms[0] = pass_ms[1] = pass_ms[2] = 0.0f;
    }
    sdfk_occgrid G = {d_sub[0], d_sub[1], d_sub[2], (unsigned)n1, (unsigned)n2, k1, k2, k0, lg(k1), lg(k2), K,
                      lg(k0) + lg(k1) + lg(k2), 1.0f / (float)K, sdfk_sel_key(level), total_cells < (1LL << 32) ? 1u : 0u, 0};
    sdfk_occclass C = {g.ax0, g.ax1, g.ax2, d_hw[0], d_hw[1], d_hw[2], (unsigned)n1, (unsigned)n2, 0, 0, level, lipschitz,
                       sdfk_sel_key(level)};
    const float* prm = x.prm;
    const float* tab = x.tab;
    const unsigned per_wave = K >= 64u ? 1u : 64u / K;          // entries of one wave (sdfk_occdev.h)
    int64_t near_total = 0;

    for (int64_t first = 0; first < total_cells; first += slab) {
        const int64_t cells = std::min(slab, total_cells - first);
        float* out = d_fraction + first;
        unsigned long long n_entries = (unsigned long long)cells;
        if (pass_ms) HIPCHK(hipEventRecord(ev.e[0], stream));
        if (skip) {
            g.start = first;
            rc = run(grid_call(p, &g, cells, d_centre, stream, mode, true));
            if (rc) return rc;
            if (pass_ms) HIPCHK(hipEventRecord(ev.e[1], stream));
            C.first = first;
            C.count = cells;
            const long long runs = occ_runs(cells);
            const unsigned blocks = (unsigned)((runs + SDFK_OCC_BLOCK / 64 - 1) / (SDFK_OCC_BLOCK / 64));
            hipLaunchKernelGGL(sdfk_occ_classify_kernel<false>, dim3(blocks), dim3(SDFK_OCC_BLOCK), 0, stream,
                               (const float*)d_centre, C, out, d_list, d_blk);
            hipLaunchKernelGGL(sdfk_select_scan_kernel, dim3(1), dim3(1024), 0, stream, d_blk, runs);
            hipLaunchKernelGGL(sdfk_occ_classify_kernel<true>, dim3(blocks), dim3(SDFK_OCC_BLOCK), 0, stream,
                               (const float*)d_centre, C, out, d_list, d_blk);
            HIPCHK(hipGetLastError());
            unsigned long long h = 0;
            HIPCHK(hipMemcpyAsync(&h, d_blk + runs, sizeof h, hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
            if (h > (unsigned long long)cells) return fail(-2, w + ": the list of near cells is longer than the slab");
            n_entries = h;
        } else if (pass_ms) {
            HIPCHK(hipEventRecord(ev.e[1], stream));
        }
        if (pass_ms) HIPCHK(hipEventRecord(ev.e[2], stream));
        near_total += (int64_t)n_entries;
        if (n_entries) {
            G.first = first;
            const unsigned long long waves = (n_entries + per_wave - 1) / per_wave;
            const unsigned blocks = (unsigned)((waves + SDFK_OCC_BLOCK / 64 - 1) / (SDFK_OCC_BLOCK / 64));
            SdfkOccList src_list = {d_list, n_entries};
            SdfkOccAll src_all = {n_entries};
            if (sk) {
                void* src = skip ? (void*)&src_list : (void*)&src_all;
                void* args[] = {&prm, &tab, src, &G, &out};
                HIPCHK(hipModuleLaunchKernel(sk->fn[skip ? 0 : 1], blocks, 1, 1, SDFK_OCC_BLOCK, 1, 1, 0, stream, args, nullptr));
            } else {
                auto launch = [&](auto src) {
                    using SRC = decltype(src);
#define SDFK_OCC_GO(NC, NV) hipLaunchKernelGGL((sdfk_occ_interp_kernel<NC, NV, SRC>), dim3(blocks), dim3(SDFK_OCC_BLOCK), 0, stream, \
                                               x.d->d_code, x.n_instr, prm, tab, x.result_reg, src, G, out)
                    SDFK_REGFILE(p, SDFK_NC, SDFK_NV, SDFK_OCC_GO);
#undef SDFK_OCC_GO
                };
                if (skip) launch(src_list);
                else launch(src_all);
                HIPCHK(hipGetLastError());
            }
        }
        if (pass_ms) {
            HIPCHK(hipEventRecord(ev.e[3], stream));
            HIPCHK(hipEventSynchronize(ev.e[3]));
            for (int k = 0; k < 3; ++k) {
                float ms = 0.0f;
                HIPCHK(hipEventElapsedTime(&ms, ev.e[k], ev.e[k + 1]));
                pass_ms[k] += ms;
            }
        }
    }
    // the sum of the counts, from the fractions: integers, whatever the order
    hipLaunchKernelGGL(sdfk_occ_total_kernel, dim3(SDFK_OCC_PARTIALS / 4), dim3(256), 0, stream, (const float*)d_fraction,
                       (long long)total_cells, (float)K, d_partial);
    HIPCHK(hipGetLastError());
    std::vector<unsigned long long> partial(SDFK_OCC_PARTIALS);
    HIPCHK(hipMemcpyAsync(partial.data(), d_partial, partial.size() * 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));                       // the tables are freed on return
    unsigned long long inside = 0;
    for (unsigned long long v : partial) inside += v;
    *inside_samples = (int64_t)inside;
    *near_cells = near_total;
    return 0;
}
