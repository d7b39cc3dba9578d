// sdfk_redistance.inc — the signed Euclidean distance of every grid point to the level set of a field, the level set
// being the crossing vertices of sdfk_mesh.inc (included at the end of sdfk.hip, after sdfk_occupancy.inc; the
// definition for users: aegolius_amd/redistance.py; the numpy form: tests/redistance_reference.py). All float32, every
// operation rounded once (the file is built with -ffp-contract=off), in the order written:
//
//   seeds   : a grid edge whose ends differ in "f <= level" (NaN: outside; the key of sdfk_sel_key) carries one seed at
//             mesh_place() along its axis — family a = the seeds of the edges along axis a. A NaN position is dropped.
//   pass 1  : along the family's axis, per grid line: g(i) = min over the line's seeds s of (x_i - s) (x_i - s), +inf
//             without a seed.
//   min-plus: along every other axis b, in increasing order: g'(j) = min over j' of g(j') + (b_j - b_j') (b_j - b_j').
//   Q       : the min over the families. The x and the y family are the same expression ((dx dx + dy dy) + dz dz, the sum
//             of two floats does not depend on their order), and a min-plus pass of a min is the min of the passes, so
//             both are merged before their common z pass: 8 passes in 3-D (x y | y x -> z, z x y), 4 in 2-D.
//   finish  : D = sqrt(Q); D = min(D, band); near band (see rd_finish_kernel); -D where f <= level.
//
// Every pass is an OUTWARD SEARCH, one lane per output point: from the point itself to both sides, source by source,
// a side ending at the first source whose distance d along the axis has d d >= best (g >= 0 and the table is strictly
// increasing, rounding is monotone: nothing farther on that side can win), beyond `band`, or at the end of the line. No
// lower envelope, no computed intersection: a min over fixed float32 expressions, so the bits are those of the
// brute-force min over all seeds, whatever the order. Work is proportional to the distance found.
//
// Pass 1 searches the line's EDGES the same way. An edge k to the right of point j has its seed at s >= x_k, so
// x_k - x_j bounds the distance from below. To the left the rounded mesh_place() may exceed x_{k+1} (by parts of the
// edge's length times 2^-24), so the bound there is x_j - U[k], U[k] = max over k' <= k of fl(x_k' + fl(x_{k'+1} -
// x_k')) >= every seed of the edges up to k (t <= 1 and rounding is monotone); the host builds U with the axis tables.
//
// Two kernels per kind of pass. rd_strided_kernel: lanes along the flat index, sources a stride apart, so every source
// read of a wave is a row segment (axes with points behind them in memory, and lines of at most RD_SHORT points).
// rd_line_kernel: the contiguous axis; a workgroup owns 256 consecutive outputs of one line and stages the sources in
// LDS in windows of RD_WIN points, ring by ring outward (its own window, then one to the left and one to the right,
// ...) until no lane has a side left (__syncthreads_or); a line of any length is walked. LDS: 8 KB (min-plus) or 12 KB
// (seeds) per 256 threads, so the 32 waves a CU holds need 64 / 96 of its 160 KB. No atomics anywhere; every output is
// stored once, with vector stores. Scratch: 2 N floats. The seed count: per-wave partial sums of the finish kernel
// (fixed grid), added on the host.
#define RD_BLOCK 256
#define RD_WIN 1024                    // sources per LDS window (a multiple of RD_BLOCK)
#define RD_SHORT 64                    // contiguous lines up to this length go through the strided kernel
#define RD_PARTIALS 4096               // waves of the finish kernel

static __device__ __forceinline__ bool rd_finite(float v) {
    return (__builtin_bit_cast(unsigned, v) & 0x7f800000u) != 0x7f800000u;
}

// one source of a min-plus pass, d >= 0 away along the axis, its value at *g: false = this side is finished
static __device__ __forceinline__ bool rd_relax(float& best, float d, const float* g, float band) {
    const float dd = d * d;
    if (d > band || dd >= best) return false;
    const float v = *g + dd;
    best = v < best ? v : best;
    return true;
}
// one edge of pass 1 (ends xa / xb with values fa / fb), d0 a lower bound of the distance to every seed from this edge on
static __device__ __forceinline__ bool rd_edge(float& best, float d0, float fa, float fb, float xa, float xb, float xj,
                                               float level, unsigned level_key, float band) {
    d0 = d0 < 0.0f ? 0.0f : d0;
    if (d0 > band || d0 * d0 >= best) return false;
    if ((sdfk_sel_key(fa) <= level_key) != (sdfk_sel_key(fb) <= level_key)) {
        const float s = mesh_place(fa, fb, xa, xb, level);
        if (!mesh_isnan(s)) {
            const float d = xj - s, dd = d * d;
            best = dd < best ? dd : best;
        }
    }
    return true;
}

struct sdfk_rdpass {
    const float* __restrict__ src;     // SEED: the field; else g of the pass before
    const float* __restrict__ other;   // nullable: a family's result that is merged in (min) as the output is stored
    float* __restrict__ dst;
    const float* __restrict__ ax;      // the axis table of the pass, len floats
    const float* __restrict__ ub;      // SEED: U, len - 1 floats
    long long n;                       // points of the grid
    long long len, inner;              // flat index = (o len + j) inner + c
    float band;                        // +inf: none
    float level;
    unsigned level_key;
};

template <bool SEED>
__global__ __launch_bounds__(RD_BLOCK) void rd_strided_kernel(sdfk_rdpass P) {
    const long long p = (long long)sdfk_bx() * RD_BLOCK + sdfk_tx();
    if (p >= P.n) return;
    const long long row = p / P.inner, o = row / P.len;
    const long long j = row - o * P.len, c = p - row * P.inner;
    const float* __restrict__ line = P.src + (o * P.len * P.inner + c);
    const float xj = P.ax[j];
    float best;
    long long lo = j - 1, hi = SEED ? j : j + 1;                // SEED: edges (lo, lo + 1) and (hi, hi + 1)
    const long long last = SEED ? P.len - 2 : P.len - 1;
    bool L = lo >= 0, R = hi <= last;
    if constexpr (SEED) {
        best = __builtin_inff();
        float fl = line[j * P.inner], fr = fl;                  // the value at the inner end of the next edge of each side
        while (L || R) {
            if (L) {
                const float fa = line[lo * P.inner];
                L = rd_edge(best, xj - P.ub[lo], fa, fl, P.ax[lo], P.ax[lo + 1], xj, P.level, P.level_key, P.band) && --lo >= 0;
                fl = fa;
            }
            if (R) {
                const float fb = line[(hi + 1) * P.inner];
                R = rd_edge(best, P.ax[hi] - xj, fr, fb, P.ax[hi], P.ax[hi + 1], xj, P.level, P.level_key, P.band) && ++hi <= last;
                fr = fb;
            }
        }
    } else {
        best = line[j * P.inner];
        while (L || R) {
            if (L) L = rd_relax(best, xj - P.ax[lo], line + lo * P.inner, P.band) && --lo >= 0;
            if (R) R = rd_relax(best, P.ax[hi] - xj, line + hi * P.inner, P.band) && ++hi <= last;
        }
    }
    if (P.other) {
        const float q = P.other[p];
        best = q < best ? q : best;
    }
    P.dst[p] = best;
}

// the contiguous axis (inner == 1): workgroup = (line, chunk of RD_BLOCK outputs), blockIdx = line * chunks + chunk
template <bool SEED>
__global__ __launch_bounds__(RD_BLOCK) void rd_line_kernel(sdfk_rdpass P, unsigned chunks) {
    __shared__ float sv[RD_WIN + 1];                            // source values of the window (SEED: one more, the last edge's end)
    __shared__ float sa[RD_WIN + 1];                            // the axis values there
    __shared__ float su[SEED ? RD_WIN : 1];                     // U
    const long long line_id = sdfk_bx() / chunks;
    const long long c0 = (long long)(sdfk_bx() - line_id * chunks) * RD_BLOCK;
    const long long j = c0 + sdfk_tx();
    const bool valid = j < P.len;
    const float* __restrict__ line = P.src + line_id * P.len;
    const long long last = SEED ? P.len - 2 : P.len - 1;        // the last source (SEED: edge) of the line
    const long long windows = (last + RD_WIN) / RD_WIN;         // ceil((last + 1) / RD_WIN)
    const long long wc = c0 / RD_WIN < windows ? c0 / RD_WIN : windows - 1;   // (SEED: the chunk of the last point alone may
                                                                              //  lie behind the last edge's window)
    const float xj = valid ? P.ax[j] : 0.0f;
    float best = SEED || !valid ? __builtin_inff() : line[j];
    long long lo = j - 1, hi = SEED ? j : j + 1;
    bool L = valid && lo >= 0, R = valid && hi <= last;

    for (long long r = 0;; ++r) {
        bool any_window = false;
        for (int side = 0; side < 2; ++side) {                  // ring r: window wc - r, then wc + r (r = 0: once)
            const long long w = side == 0 ? wc - r : wc + r;
            if (w < 0 || w >= windows || (side == 1 && r == 0)) continue;      // (workgroup-uniform)
            any_window = true;
            const long long w0 = w * RD_WIN;
            const long long w1 = w0 + RD_WIN <= last + 1 ? w0 + RD_WIN : last + 1;   // sources [w0, w1)
            __syncthreads();                                    // the window before is no longer read
            for (long long t = sdfk_tx(); t <= w1 - w0; t += RD_BLOCK) {
                if (w0 + t < P.len) {
                    sv[t] = line[w0 + t];
                    sa[t] = P.ax[w0 + t];
                }
                if constexpr (SEED)
                    if (t < w1 - w0) su[t] = P.ub[w0 + t];
            }
            __syncthreads();
            for (;;) {
                const bool l = L && lo >= w0 && lo < w1, rt = R && hi >= w0 && hi < w1;
                if (!l && !rt) break;
                if constexpr (SEED) {
                    if (l) {
                        const long long k = lo - w0;
                        L = rd_edge(best, xj - su[k], sv[k], sv[k + 1], sa[k], sa[k + 1], xj, P.level, P.level_key, P.band) &&
                            --lo >= 0;
                    }
                    if (rt) {
                        const long long k = hi - w0;
                        R = rd_edge(best, sa[k] - xj, sv[k], sv[k + 1], sa[k], sa[k + 1], xj, P.level, P.level_key, P.band) &&
                            ++hi <= last;
                    }
                } else {
                    if (l) L = rd_relax(best, xj - sa[lo - w0], sv + (lo - w0), P.band) && --lo >= 0;
                    if (rt) R = rd_relax(best, sa[hi - w0] - xj, sv + (hi - w0), P.band) && ++hi <= last;
                }
            }
        }
        if (!any_window || !__syncthreads_or(L || R)) break;    // (both workgroup-uniform)
    }
    if (!valid) return;
    const long long p = line_id * P.len + j;
    if (P.other) {
        const float q = P.other[p];
        best = q < best ? q : best;
    }
    P.dst[p] = best;
}

struct sdfk_rdfinish {
    const float* __restrict__ field;
    const float* __restrict__ ax0;
    const float* __restrict__ ax1;
    const float* __restrict__ ax2;
    long long n;
    unsigned n1, n2;                   // (n0 = n / (n1 n2))
    float band, level;
    unsigned level_key;
    int near;                          // 1: the near-band estimate
};

// One gradient component at index i of an axis of n points (n >= 2), stride s floats between its points: the central
// difference inside, the one-sided one at the ends. *ok stays true only while every value read is finite.
static __device__ __forceinline__ float rd_gradient(const float* __restrict__ f, const float* __restrict__ ax, long long i,
                                                    long long n, long long s, bool* ok) {
    const long long a = i > 0 ? i - 1 : i, b = i < n - 1 ? i + 1 : i;
    const float fa = f[(a - i) * s], fb = f[(b - i) * s];
    *ok = *ok && rd_finite(fa) && rd_finite(fb);
    return (fb - fa) / (ax[b] - ax[a]);
}

// q (in place): Q of the last family, merged with `other` (nullable) -> the signed distance. A fixed grid of RD_PARTIALS
// waves strides over the points; wave w leaves the seeds of its points' own (+x, +y, +z) edges in partial[w].
// Near band, at every point that is an end of a crossing edge (a neighbour along an axis differs in "f <= level"):
//     g_a = rd_gradient per axis of at least 2 points;  m = sqrt((gx gx + gy gy) + gz gz);  e = |f - level| / m
// and D = min(e, D) if every field value used, m, |f - level| and e are finite and m > 0; else the point keeps D. (Bit
// tests before the arithmetic: no NaN is ever computed, -fno-honor-nans leaves that undefined.)
__global__ __launch_bounds__(RD_BLOCK) void rd_finish_kernel(float* __restrict__ q, const float* __restrict__ other, sdfk_rdfinish F,
                                                             unsigned long long* __restrict__ partial) {
    const unsigned lane = sdfk_tx() & 63u;
    const long long wave = (long long)sdfk_bx() * (RD_BLOCK / 64) + (sdfk_tx() >> 6);
    const long long n0 = F.n / ((long long)F.n1 * F.n2), s0 = (long long)F.n1 * F.n2, s1 = F.n2;
    unsigned long long seeds = 0;                               // (wave-uniform)
    for (long long p = wave * 64 + lane; p < F.n; p += (long long)RD_PARTIALS * 64) {
        const long long row = p / F.n2, i0 = row / F.n1;
        const long long i2 = p - row * F.n2, i1 = row - i0 * F.n1;
        const float* __restrict__ fp = F.field + p;
        const float f = *fp;
        const bool in = sdfk_sel_key(f) <= F.level_key;
        auto differs = [&](long long off) { return (sdfk_sel_key(fp[off]) <= F.level_key) != in; };
        const bool c0 = i0 + 1 < n0 && differs(s0), c1 = i1 + 1 < F.n1 && differs(s1), c2 = i2 + 1 < F.n2 && differs(1);
        seeds += (unsigned)(__popcll(__ballot(c0)) + __popcll(__ballot(c1)) + __popcll(__ballot(c2)));
        float Q = q[p];
        if (other) {
            const float o = other[p];
            Q = o < Q ? o : Q;
        }
        float D = __builtin_sqrtf(Q);                           // correctly rounded (the build's default for sqrtf and /)
        D = F.band < D ? F.band : D;
        if (F.near && (c0 || c1 || c2 || (i0 > 0 && differs(-s0)) || (i1 > 0 && differs(-s1)) || (i2 > 0 && differs(-1)))) {
            bool ok = rd_finite(f);
            const float g0 = rd_gradient(fp, F.ax0, i0, n0, s0, &ok);
            const float g1 = rd_gradient(fp, F.ax1, i1, F.n1, s1, &ok);
            float mm = g0 * g0 + g1 * g1;
            if (F.n2 > 1u) {
                const float g2 = rd_gradient(fp, F.ax2, i2, F.n2, 1, &ok);
                mm = mm + g2 * g2;
            }
            if (ok) {
                const float m = __builtin_sqrtf(mm), num = __builtin_fabsf(f - F.level);
                if (rd_finite(m) && m > 0.0f && rd_finite(num)) {
                    const float e = num / m;
                    if (rd_finite(e)) D = e < D ? e : D;
                }
            }
        }
        q[p] = in ? -D : D;
    }
    if (lane == 0u) partial[wave] = seeds;
}

// ---- host side ----------------------------------------------------------------------------------
extern "C" size_t sdfk_field_redistance_scratch(int64_t n0, int64_t n1, int64_t n2) {
    if (n0 < 1 || n1 < 1 || n2 < 1) return 0;
    return (size_t)(n0 * n1 * n2) * 2 * sizeof(float);
}

struct RdEvents {
    hipEvent_t e[SDFK_REDISTANCE_PASSES + 1] = {};
    ~RdEvents() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
};
struct RdTables {
    float* d = nullptr;
    ~RdTables() {
        if (d) (void)hipFree(d);
    }
};

extern "C" int sdfk_field_redistance(const float* d_field, const float* ax0, int64_t n0, const float* ax1, int64_t n1,
                                     const float* ax2, int64_t n2, float level, float band, int near, float* d_out,
                                     void* d_scratch, int64_t* seeds, float* pass_ms, void* stream_) {
    const std::string w = "sdfk_field_redistance";
    if (!d_field || !d_out || !d_scratch) return fail(-1, w + ": null field, output or scratch pointer");
    if (d_field == d_out) return fail(-1, w + ": the output must not be the field");
    if (!ax0 || !ax1 || (n2 > 1 && !ax2)) return fail(-1, w + ": null axis table");
    if (n0 < 2 || n1 < 2 || n2 < 1 || n0 > 0x7fffffff || n1 > 0x7fffffff || n2 > 0x7fffffff)
        return fail(-1, w + ": two or three axes of 2 to 2^31 - 1 points (a 2-D grid has n2 = 1)");
    if (occ_is_nan(level)) return fail(-1, w + ": the level is NaN");
    if (occ_is_nan(band) || (band > 0.0f && !occ_is_finite(band))) return fail(-1, w + ": the band is NaN or infinite");
    if (near != 0 && near != 1) return fail(-1, w + ": near is 0 (seeds only) or 1 (gradient estimate)");
    if (!seeds) return fail(-1, w + ": null seed counter");
    const int64_t dims[3] = {n0, n1, n2};
    const float* ax[3] = {ax0, ax1, ax2};
    const int D = n2 > 1 ? 3 : 2;
    if ((double)n0 * (double)n1 * (double)n2 > (double)(1LL << 40)) return fail(-1, w + ": more than 2^40 points");
    const int64_t n = n0 * n1 * n2;
    for (int a = 0; a < D; ++a)
        for (int64_t i = 1; i < dims[a]; ++i)
            if (!(ax[a][i] > ax[a][i - 1]) || !occ_is_finite(ax[a][i]) || !occ_is_finite(ax[a][i - 1]))
                return fail(-1, w + ": axis " + std::to_string(a) + " is not finite and strictly increasing");

    // device tables: per axis the points, then U (see the head of the file); then the finish kernel's partial sums
    std::vector<float> host;
    size_t at_ax[3] = {0, 0, 0}, at_ub[3] = {0, 0, 0};
    for (int a = 0; a < D; ++a) {
        at_ax[a] = host.size();
        host.insert(host.end(), ax[a], ax[a] + dims[a]);
        at_ub[a] = host.size();
        float top = -__builtin_inff();
        for (int64_t k = 0; k + 1 < dims[a]; ++k) {
            volatile float step = ax[a][k + 1] - ax[a][k];     // (volatile: each operation rounded to float32 on its own)
            volatile float end = ax[a][k] + step;
            top = end > top ? end : top;
            host.push_back(top);
        }
    }
    const size_t table_bytes = (host.size() * sizeof(float) + 255) / 256 * 256;
    hipStream_t stream = (hipStream_t)stream_;
    RdTables tab;
    HIPCHK(hipMalloc(&tab.d, table_bytes + RD_PARTIALS * sizeof(unsigned long long)));
    HIPCHK(hipMemcpyAsync(tab.d, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, stream));
    unsigned long long* d_partial = (unsigned long long*)((char*)tab.d + table_bytes);

    float* S1 = (float*)d_scratch;
    float* S2 = S1 + n;
    const float bandv = band > 0.0f ? band : __builtin_inff();
    const unsigned key = sdfk_sel_key(level);
    RdEvents ev;
    int n_ev = 0;
    if (pass_ms) {
        for (int k = 0; k < SDFK_REDISTANCE_PASSES; ++k) pass_ms[k] = 0.0f;
        for (hipEvent_t& x : ev.e) HIPCHK(hipEventCreate(&x));
        HIPCHK(hipEventRecord(ev.e[n_ev++], stream));
    }
    // one pass along axis a: seed = pass 1 of family a (src the field), else min-plus
    auto pass = [&](int a, bool seed, const float* src, const float* other, float* dst) -> int {
        int64_t inner = 1;
        for (int b = a + 1; b < D; ++b) inner *= dims[b];
        sdfk_rdpass P = {src, other, dst, tab.d + at_ax[a], tab.d + at_ub[a], (long long)n, (long long)dims[a], (long long)inner,
                         bandv, level, key};
        if (inner > 1 || dims[a] <= RD_SHORT) {
            const int64_t blocks = (n + RD_BLOCK - 1) / RD_BLOCK;
            if (blocks > 0x7fffffffLL) return fail(-1, w + ": the grid is too large for one launch");
            if (seed) hipLaunchKernelGGL(rd_strided_kernel<true>, dim3((unsigned)blocks), dim3(RD_BLOCK), 0, stream, P);
            else hipLaunchKernelGGL(rd_strided_kernel<false>, dim3((unsigned)blocks), dim3(RD_BLOCK), 0, stream, P);
        } else {
            const int64_t chunks = (dims[a] + RD_BLOCK - 1) / RD_BLOCK, blocks = (n / dims[a]) * chunks;
            if (blocks > 0x7fffffffLL) return fail(-1, w + ": the grid is too large for one launch");
            if (seed) hipLaunchKernelGGL(rd_line_kernel<true>, dim3((unsigned)blocks), dim3(RD_BLOCK), 0, stream, P, (unsigned)chunks);
            else hipLaunchKernelGGL(rd_line_kernel<false>, dim3((unsigned)blocks), dim3(RD_BLOCK), 0, stream, P, (unsigned)chunks);
        }
        HIPCHK(hipGetLastError());
        if (pass_ms) HIPCHK(hipEventRecord(ev.e[n_ev++], stream));
        return 0;
    };
    int rc = 0;
    const float* other = nullptr;                               // what the finish kernel merges in
    if ((rc = pass(0, true, d_field, nullptr, S1)) || (rc = pass(1, false, S1, nullptr, S2)) ||        // x family: x, y
        (rc = pass(1, true, d_field, nullptr, S1)) || (rc = pass(0, false, S1, S2, d_out)))           // y family: y, x; merged
        return rc;
    if (D == 3) {
        if ((rc = pass(2, false, d_out, nullptr, S2)) ||                                             // their z pass
            (rc = pass(2, true, d_field, nullptr, d_out)) || (rc = pass(0, false, d_out, nullptr, S1)) ||   // z family: z, x, y
            (rc = pass(1, false, S1, nullptr, d_out)))
            return rc;
        other = S2;
    }
    sdfk_rdfinish F = {d_field, tab.d + at_ax[0], tab.d + at_ax[1], D == 3 ? tab.d + at_ax[2] : nullptr, (long long)n,
                       (unsigned)n1, (unsigned)n2, bandv, level, key, near};
    hipLaunchKernelGGL(rd_finish_kernel, dim3(RD_PARTIALS / (RD_BLOCK / 64)), dim3(RD_BLOCK), 0, stream, d_out, other, F, d_partial);
    HIPCHK(hipGetLastError());
    if (pass_ms) HIPCHK(hipEventRecord(ev.e[n_ev++], stream));
    std::vector<unsigned long long> partial(RD_PARTIALS);
    HIPCHK(hipMemcpyAsync(partial.data(), d_partial, partial.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));                       // the tables are freed on return
    unsigned long long total = 0;
    for (unsigned long long v : partial) total += v;
    *seeds = (int64_t)total;
    if (pass_ms)
        for (int k = 0; k + 1 < n_ev; ++k) HIPCHK(hipEventElapsedTime(&pass_ms[k], ev.e[k], ev.e[k + 1]));
    return 0;
}
