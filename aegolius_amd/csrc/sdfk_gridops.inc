// sdfk_gridops.inc — grid-neighbourhood operators on a field resident in HBM (included by sdfk.hip).
//
// The three modifications of the reference that are NOT pointwise (SURVEY §8(f).1): they reshape the field
// to the grid (smarter_reshape, C/helper_functions.py:96-148) and look at neighbours:
//   conv_averaging       C/modifications.py:1589-1615 -> C/post_processing.py:561-600  scipy.ndimage.convolve, box kernel
//   conv_edge_detection  C/modifications.py:1617-1637 -> C/post_processing.py:603-623  3x3(x1) Laplacian-like kernel
//   signed               C/modifications.py:220-275   scan-line parity of boundary crossings along axes 0 and 1
// scipy.ndimage.convolve(u, w) with its defaults (mode="reflect", origin 0), as measured here against scipy 1.15:
//   out[i] = sum_j w[j] * u_ext[i + size//2 - j],  u_ext = (d c b a | a b c d | d c b a)
// so a box kernel of `size` taps covers the offsets -((size-1)//2) .. size//2.
// Layout: flat index (i*n1 + j)*n2 + k, exactly the (N,) field of the evaluation kernels; a 2-D field has n2 = 1.

static __device__ __forceinline__ int sdfk_reflect(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
}

struct GridDims {
    int n0, n1, n2;
};
static __device__ __forceinline__ bool sdfk_unflatten(long long t, const GridDims& d, int& i, int& j, int& k) {
    const long long total = (long long)d.n0 * d.n1 * d.n2;
    if (t >= total) return false;
    k = (int)(t % d.n2);
    const long long r = t / d.n2;
    j = (int)(r % d.n1);
    i = (int)(r / d.n1);
    return true;
}

// Launch geometry of the stencil kernels: sdfk_bz() / .y = i / j, threads along k (no integer division); a flat
// field (n2 == 1) is relabelled (1, n0, n1) by the host so that the threads still run along the contiguous axis.
// reflect an index that lies at most n outside [0, n) — branch-free (two selects); FAST = false: any index
// (integer modulo: only when a kernel is wider than the field)
template <bool FAST>
static __device__ __forceinline__ int sdfk_wrap(int i, int n) {
    if (FAST) return i < 0 ? -1 - i : (i >= n ? 2 * n - 1 - i : i);
    return sdfk_reflect(i, n);
}
// Box sum over k0 x k1 x k2 taps, accumulated in float64 in a fixed order (axis 0 outermost, then 1, then 2) and
// rounded once to fp32. A workgroup owns 4 x 64 outputs of one i-plane and stages the (4 + k1 - 1) x (64 + k2 - 1)
// halo tile of as many of the k0 planes as fit in LDS: ~1.5 global loads per output and plane instead of k1*k2.
//   edge = 0: out = sum * inv_norm                      (conv_averaging)
//   edge = 1: out = 9 * centre - sum over the 3x3 box   (= [[-1,-1,-1],[-1,8,-1],[-1,-1,-1]], conv_edge_detection)
#define SDFK_BOX_TJ 4
#define SDFK_BOX_TK 64
// K2C: the innermost kernel extent as a compile-time constant (0 = any, taken from k2): with it the tap loop is
// straight-line ds_read_b64 + v_add_f64; with run-time bounds the loop bookkeeping was ~50 instructions per tap.
template <bool FAST, int K2C>
__global__ __launch_bounds__(256) void sdfk_box_kernel(const float* __restrict__ in, float* __restrict__ out, GridDims d,
                                                       int k0, int k1, int k2_, double inv_norm, int edge, int pc) {
    const int k2 = K2C ? K2C : k2_;
    extern __shared__ double tile[];   // converted once at fill time: v_cvt_f64_f32 runs at a fraction of the f64 add rate
    const int tk = sdfk_tx() & 63, tj = sdfk_tx() >> 6;
    const int i = sdfk_bz(), j0 = sdfk_by() * SDFK_BOX_TJ;
    const int lo0 = (k0 - 1) / 2, lo1 = (k1 - 1) / 2, lo2 = (k2 - 1) / 2;
    const int hj = SDFK_BOX_TJ + k1 - 1, hk = SDFK_BOX_TK + k2 - 1;
    const int j = j0 + tj;
  // a workgroup walks along k: one launch slot per 4 rows
  for (int kb = sdfk_bx() * SDFK_BOX_TK; kb < d.n2; kb += sdfk_gx() * SDFK_BOX_TK) {
    const int k = kb + tk;
    const bool live = j < d.n1 && k < d.n2;
    const int plane = hj * hk;
    double acc = 0.0;
    for (int a0 = 0; a0 < k0; a0 += pc) {                     // `pc` planes of halo fit the LDS tile at a time
        const int na = min(pc, k0 - a0);
        // fill: (plane, row) pairs are dealt to the 4 waves, a wave reads a halo row 64 points at a time; no integer
        // division anywhere (a flat index cost ~80 VALU instructions per element)
        for (int ar = tj; ar < na * hj; ar += SDFK_BOX_TJ) {
            int a = 0, jj = ar;
            while (jj >= hj) { jj -= hj; ++a; }                                                  // na is small
            const long long ia = sdfk_wrap<FAST>(i + a0 + a - lo0, d.n0);
            const long long gj = sdfk_wrap<FAST>(min(j0 + jj - lo1, d.n1 - 1 + k1 / 2), d.n1);   // (cells past that
            const float* row = in + (ia * d.n1 + gj) * d.n2;                                     //  feed no live output)
#pragma unroll 2
            for (int kk = tk; kk < hk; kk += SDFK_BOX_TK)
                tile[a * plane + jj * hk + kk] = (double)row[sdfk_wrap<FAST>(min(kb + kk - lo2, d.n2 - 1 + k2 / 2), d.n2)];
        }
        __syncthreads();
        if (live)
            for (int a = 0; a < na; ++a)
                for (int b = 0; b < k1; ++b) {
                    const double* t = tile + a * plane + (tj + b) * hk + tk;
                    if (K2C) {
#pragma unroll
                        for (int c = 0; c < K2C; ++c) acc += t[c];
                    } else {
                        for (int c = 0; c < k2; ++c) acc += t[c];
                    }
                }
        __syncthreads();
    }
    if (live) {
        const long long t = ((long long)i * d.n1 + j) * d.n2 + k;
        out[t] = edge ? (float)(9.0 * (double)in[t] - acc) : (float)(acc * inv_norm);
    }
  }
}
// Marching variant (k0 <= 7, the usual case): a workgroup owns 8 rows x 64 columns and marches along i. Every plane's
// halo tile is loaded ONCE (the kernel above reloads it for each of the k0 outputs that use it); a thread adds up
// the k1 x k2 window of its 2 rows — the k2-wide row sums are shared by the rows that overlap — and keeps the last
// K0 plane sums in registers: out[i] = the K0 plane sums in order of i. The tile is double-buffered: the next
// plane is fetched while this one is summed, one barrier per plane.
#define SDFK_BOXM_R 2                       // rows per thread
#define SDFK_BOXM_TJ (4 * SDFK_BOXM_R)
#define SDFK_BOXM_SEG 32                    // output planes per workgroup
template <int K0C, int K2C>
__global__ __launch_bounds__(256) void sdfk_box_march_kernel(const float* __restrict__ in, float* __restrict__ out, GridDims d,
                                                             int k1, int k2_, double inv_norm, int edge, int seg) {
    const int k2 = K2C ? K2C : k2_;
    extern __shared__ double tile[];
    const int tk = sdfk_tx() & 63, tj = sdfk_tx() >> 6;
    const int kb = sdfk_bx() * SDFK_BOX_TK, j0 = sdfk_by() * SDFK_BOXM_TJ, i0 = sdfk_bz() * seg;
    const int i1 = min(i0 + seg, d.n0);
    const int lo0 = (K0C - 1) / 2, lo1 = (k1 - 1) / 2, lo2 = (k2 - 1) / 2, hi0 = K0C - 1 - lo0;
    const int hj = SDFK_BOXM_TJ + k1 - 1, hk = SDFK_BOX_TK + k2 - 1, plane = hj * hk;
    const int k = kb + tk, jbase = j0 + tj * SDFK_BOXM_R;
    // the halo cells this thread fetches for every plane (the same (row, column) pairs each time): up to 4
    const int cells = plane;
    long long off[4];
    int slot[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = sdfk_tx() + q * 256;
        slot[q] = c < cells ? c : -1;
        const int jj = c / hk, kk = c - jj * hk;
        const long long gj = sdfk_wrap<true>(min(j0 + jj - lo1, d.n1 - 1 + k1 / 2), d.n1);
        off[q] = gj * d.n2 + sdfk_wrap<true>(min(kb + kk - lo2, d.n2 - 1 + k2 / 2), d.n2);
    }
    const long long pstride = (long long)d.n1 * d.n2;
    float pre[4];
    auto fetch = [&](int e) {                                  // extended plane e (may lie outside: reflected)
        const float* src = in + (long long)sdfk_wrap<true>(e, d.n0) * pstride;
#pragma unroll
        for (int q = 0; q < 4; ++q) pre[q] = slot[q] >= 0 ? src[off[q]] : 0.0f;
    };
    double ring[SDFK_BOXM_R][K0C];
#pragma unroll
    for (int r = 0; r < SDFK_BOXM_R; ++r)
#pragma unroll
        for (int a = 0; a < K0C; ++a) ring[r][a] = 0.0;
    const int e0 = i0 - lo0, e1 = i1 - 1 + hi0;                // planes this segment reads
    fetch(e0);
    int buf = 0;
    for (int e = e0; e <= e1; ++e, buf ^= 1) {
        double* t = tile + buf * plane;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (slot[q] >= 0) t[slot[q]] = (double)pre[q];
        if (e < e1) fetch(e + 1);                              // in flight while this plane is summed
        __syncthreads();
        // k2-wide sums of the rows this thread's outputs touch, then the k1 of them per output
        double ps[SDFK_BOXM_R];
#pragma unroll
        for (int r = 0; r < SDFK_BOXM_R; ++r) ps[r] = 0.0;
        for (int b = 0; b < SDFK_BOXM_R + k1 - 1; ++b) {
            const double* row = t + (tj * SDFK_BOXM_R + b) * hk + tk;
            double rs = 0.0;
            if (K2C) {
#pragma unroll
                for (int c = 0; c < K2C; ++c) rs += row[c];
            } else {
                for (int c = 0; c < k2; ++c) rs += row[c];
            }
#pragma unroll
            for (int r = 0; r < SDFK_BOXM_R; ++r)
                if (b >= r && b < r + k1) ps[r] += rs;
        }
#pragma unroll
        for (int r = 0; r < SDFK_BOXM_R; ++r) {
#pragma unroll
            for (int a = 0; a + 1 < K0C; ++a) ring[r][a] = ring[r][a + 1];
            ring[r][K0C - 1] = ps[r];
        }
        const int i = e - hi0;                                 // the output plane completed by this step
        if (i >= i0 && k < d.n2) {
#pragma unroll
            for (int r = 0; r < SDFK_BOXM_R; ++r) {
                const int j = jbase + r;
                if (j >= d.n1) break;
                double acc = 0.0;
#pragma unroll
                for (int a = 0; a < K0C; ++a) acc += ring[r][a];
                const long long p = ((long long)i * d.n1 + j) * d.n2 + k;
                out[p] = edge ? (float)(9.0 * (double)in[p] - acc) : (float)(acc * inv_norm);
            }
        }
    }
}

// Which kernel a box launch takes, decided in ONE place: the launch below and sdfk_debug_box_variant (the tests' view of
// the dispatch) both read it, so the query cannot drift from the launch.
struct BoxVariant {
    bool march, fast, flat;
    int k0c, k2c;              // template arguments (k0c: marching kernel only; k2c 0 = run-time k2)
    int pc, chunks;            // tiled: halo planes per LDS chunk and ceil(k0 / pc); marching: planes per segment, 1
    GridDims d;                // the grid and the kernel as the device kernels see them: a flat field (n2 == 1) is
    int k0, k1, k2;            //   relabelled (1, n0, n1) and its kernel (1, k0, k1); k2 is folded away
    dim3 grid;
    size_t lds;
};
static int box_variant(GridDims d, int k0, int k1, int k2, BoxVariant* v) {
    v->flat = d.n2 == 1;
    if (v->flat) {                                            // flat field: threads along its contiguous axis
        d = GridDims{1, d.n0, d.n1};
        k2 = k1; k1 = k0; k0 = 1;
    }
    v->d = d;
    v->k0 = k0; v->k1 = k1; v->k2 = k2;
    v->fast = k0 / 2 <= d.n0 && k1 / 2 <= d.n1 && k2 / 2 <= d.n2;       // taps reach at most one field width outside
    const int hjm = SDFK_BOXM_TJ + k1 - 1, hk = SDFK_BOX_TK + k2 - 1;
    const unsigned kt = (unsigned)((d.n2 + SDFK_BOX_TK - 1) / SDFK_BOX_TK);
    v->march = v->fast && k0 <= 7 && k0 != 6 && (long long)hjm * hk <= 1024    // 4 halo cells per thread; reflections one field deep
               && (d.n1 + SDFK_BOXM_TJ - 1) / SDFK_BOXM_TJ <= 65535 && (d.n0 + SDFK_BOXM_SEG - 1) / SDFK_BOXM_SEG <= 65535
               && !getenv("SDFK_BOX_NO_MARCH");                          // A/B switch for the bench tool
    if (v->march) {
        int seg = SDFK_BOXM_SEG;
        if (const char* e = getenv("SDFK_BOXM_SEG")) seg = std::max(1, atoi(e));             // experiments
        v->k0c = k0;
        v->k2c = (k2 == 1 || k2 == 3 || k2 == 5) ? k2 : 0;
        v->pc = seg;
        v->chunks = 1;
        v->grid = dim3(kt, (unsigned)((d.n1 + SDFK_BOXM_TJ - 1) / SDFK_BOXM_TJ), (unsigned)((d.n0 + seg - 1) / seg));
        v->lds = (size_t)2 * hjm * hk * sizeof(double);
        return 0;
    }
    const long long plane = (long long)(SDFK_BOX_TJ + k1 - 1) * hk;
    if (plane > 7500) return fail(-1, "grid operator: kernel too wide for the LDS tile ((k1 + 3) * (k2 + 63) <= 7500)");
    v->pc = (int)std::max<long long>(1, std::min<long long>(k0, 7500 / plane));              // planes per LDS chunk
    v->chunks = (k0 + v->pc - 1) / v->pc;
    v->lds = (size_t)v->pc * plane * sizeof(double);
    const unsigned gy = (unsigned)((d.n1 + SDFK_BOX_TJ - 1) / SDFK_BOX_TJ);
    if (d.n0 > 65535 || gy > 65535) return fail(-1, "grid operator: grid dimension beyond the launch limits");
    // workgroups in flight: enough to fill the chip several times over, few enough that each walks several k-tiles
    const long long rows = (long long)gy * d.n0;
    const unsigned gx = (unsigned)std::max<long long>(1, std::min<long long>(kt, (16384 + rows - 1) / rows));
    v->grid = dim3(gx, gy, (unsigned)d.n0);
    v->k0c = 0;
    v->k2c = !v->fast ? 0 : (k2 <= 5 || k2 == 7) ? k2 : 0;
    return 0;
}

template <int K0C>
static void box_march_go(const float* src, float* dst, const BoxVariant& v, double inv, int edge, hipStream_t stream) {
#define SDFK_BOXM_GO(K2) hipLaunchKernelGGL((sdfk_box_march_kernel<K0C, K2>), v.grid, dim3(256), v.lds, stream, src, dst, v.d, v.k1, v.k2, inv, edge, v.pc)
    switch (v.k2c) {
        case 1: SDFK_BOXM_GO(1); break;
        case 3: SDFK_BOXM_GO(3); break;
        case 5: SDFK_BOXM_GO(5); break;
        default: SDFK_BOXM_GO(0); break;
    }
#undef SDFK_BOXM_GO
}

static void box_launch(const float* src, float* dst, const BoxVariant& v, double inv, int edge, hipStream_t stream) {
    if (v.march) {
        switch (v.k0c) {
            case 1: box_march_go<1>(src, dst, v, inv, edge, stream); break;
            case 2: box_march_go<2>(src, dst, v, inv, edge, stream); break;
            case 3: box_march_go<3>(src, dst, v, inv, edge, stream); break;
            case 4: box_march_go<4>(src, dst, v, inv, edge, stream); break;
            case 5: box_march_go<5>(src, dst, v, inv, edge, stream); break;
            default: box_march_go<7>(src, dst, v, inv, edge, stream); break;
        }
        return;
    }
#define SDFK_BOX_GO(F, K) hipLaunchKernelGGL((sdfk_box_kernel<F, K>), v.grid, dim3(256), v.lds, stream, src, dst, v.d, v.k0, v.k1, v.k2, inv, edge, v.pc)
    if (!v.fast) SDFK_BOX_GO(false, 0);
    else switch (v.k2c) {
        case 1: SDFK_BOX_GO(true, 1); break;
        case 2: SDFK_BOX_GO(true, 2); break;
        case 3: SDFK_BOX_GO(true, 3); break;
        case 4: SDFK_BOX_GO(true, 4); break;
        case 5: SDFK_BOX_GO(true, 5); break;
        case 7: SDFK_BOX_GO(true, 7); break;
        default: SDFK_BOX_GO(true, 0); break;
    }
#undef SDFK_BOX_GO
}

// ---- signed ------------------------------------------------------------------------------------------------
// boundary = s < min(spacings); along an axis: chu[i] = boundary[i] & ~boundary[i-1] (i >= 1),
// chuu[i] = boundary[i] & ~boundary[i+1] (i <= n-2); mark = cumsum(chu), fmark = flip(cumsum(chuu)) — the
// cumulative sum is flipped, it is not a reverse sum (C/modifications.py:250-254) —
// inside_axis = (mark odd) | (fmark odd); interior = inside_0 & inside_1.
// Everything between the boundary test and the sign flip is one BIT per point, so it is kept as bit planes: the k axis
// (the contiguous one, never scanned) is packed 32 points to a word, and every step below is word-wide logic on
// arrays of n0 x n1 x kw words (kw = ceil(n2/32)) — 1/32 of the field's bytes, which stay in L2. The field itself is
// read once for the test (4 B/point) and read+written once for the flip (8 B/point).
//
// 1. boundary bits: a wave takes 64 consecutive k of SDFK_BITS_LINES lines at a time (one line per wave was bound by
//    wave launches: 0.39 ms at 513^3 for 0.54 GB) -> a ballot is the two words of a line. The same pass takes the field's
//    minimum for the "already signed" test (C/modifications.py:236-237) when `key` is given.
//    `mask` (optional): the test already done, 1 byte per point (slabs of a sharded grid exchange it, DESIGN §9.5)
#define SDFK_BITS_LINES 8
// fp32 order-preserving integer key (for atomicMin)
static __device__ __forceinline__ unsigned sdfk_fkey(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__global__ __launch_bounds__(256) void sdfk_signed_bits_kernel(const float* __restrict__ s, const unsigned char* __restrict__ mask,
                                                               unsigned* __restrict__ bits, long long lines, int n2, int kw,
                                                               float sep_min, unsigned* __restrict__ key) {
    const unsigned chunks = (unsigned)(n2 + 63) >> 6, lane = sdfk_tx() & 63;
    const unsigned groups = (unsigned)((lines + SDFK_BITS_LINES - 1) / SDFK_BITS_LINES), total = groups * chunks;
    unsigned best = 0xffffffffu;
    // a fixed number of waves walks the (line group, chunk) pairs: short-lived waves — one pair each — reached 2 TB/s
    for (unsigned wave = sdfk_bx() * 4 + (sdfk_tx() >> 6); wave < total; wave += sdfk_gx() * 4) {
        const unsigned group = wave / chunks, chunk = wave - group * chunks;
        const int k = (int)(chunk * 64 + lane);
        const long long line0 = (long long)group * SDFK_BITS_LINES;
        float v[SDFK_BITS_LINES];
#pragma unroll
        for (int u = 0; u < SDFK_BITS_LINES; ++u) {
            const long long at = (line0 + u) * n2 + k;
            const bool in = k < n2 && line0 + u < lines;
            // (a mask byte becomes a value on the right side of the threshold; points outside the grid are never boundary)
            v[u] = in ? (mask ? (mask[at] ? sep_min - 1.0f : sep_min) : s[at]) : sep_min;
        }
        unsigned word = 0u;
#pragma unroll
        for (int u = 0; u < SDFK_BITS_LINES; ++u) {
            const unsigned long long b = __ballot(v[u] < sep_min);
            // lane 2u keeps the low word of line u, lane 2u + 1 the high one: the 16 words leave in ONE store instruction
            // (lane 0 storing them one by one cost 16 vector-memory issues per wave)
            if ((lane >> 1) == (unsigned)u) word = (lane & 1) ? (unsigned)(b >> 32) : (unsigned)b;
            if (key && k < n2 && line0 + u < lines)              // NaN (tested on the bits: -fno-honor-nans) counts as negative
                best = (__float_as_uint(v[u]) & 0x7fffffffu) > 0x7f800000u ? 0u : min(best, sdfk_fkey(v[u]));
        }
        if (lane < 2 * SDFK_BITS_LINES && line0 + (lane >> 1) < lines && 2 * chunk + (lane & 1) < (unsigned)kw)
            bits[(line0 + (lane >> 1)) * kw + 2 * chunk + (lane & 1)] = word;
    }
    if (key) {
        for (int off = 32; off > 0; off >>= 1) best = min(best, (unsigned)__shfl_down((int)best, off));
        // (one address: a quarter of a million atomics serialise — 3.4 ms at 513^3 — so a wave looks before it writes)
        if (lane == 0 && best < __atomic_load_n(key, __ATOMIC_RELAXED)) atomicMin(key, best);
    }
}
// 2. the two scans: one thread per (line of the scan axis, word); m = parity of mark, f = parity of cumsum(chuu),
//    both inclusive of the point. A line is walked serially, so the loads of the next SDFK_SCAN_AHEAD steps are issued
//    together (there are only a few thousand lines: nothing else hides the latency).
#define SDFK_SCAN_AHEAD 16
__global__ __launch_bounds__(256) void sdfk_signed_scan_kernel(const unsigned* __restrict__ bits, unsigned* __restrict__ m0,
                                                               unsigned* __restrict__ f0, unsigned* __restrict__ m1,
                                                               unsigned* __restrict__ f1, int n0, int n1, int kw, unsigned blocks0) {
    const int axis = sdfk_bx() < blocks0 ? 0 : 1;             // the first blocks0 workgroups scan axis 0, the rest axis 1
    unsigned* __restrict__ pm = axis == 0 ? m0 : m1;
    unsigned* __restrict__ pf = axis == 0 ? f0 : f1;
    const long long t = (long long)(sdfk_bx() - (axis ? blocks0 : 0u)) * 256 + sdfk_tx();
    const int len = axis == 0 ? n0 : n1;
    const long long lines = (long long)(axis == 0 ? n1 : n0) * kw;
    if (t >= lines) return;
    long long base, step;
    if (axis == 0) {
        base = t;                                              // (j, w) flattened
        step = (long long)n1 * kw;
    } else {
        const long long i = t / kw, w = t % kw;
        base = i * n1 * kw + w;
        step = kw;
    }
    unsigned m = 0, f = 0, prev = 0, cur = bits[base];
    for (int i0 = 0; i0 < len; i0 += SDFK_SCAN_AHEAD) {
        unsigned ahead[SDFK_SCAN_AHEAD];
#pragma unroll
        for (int u = 0; u < SDFK_SCAN_AHEAD; ++u) ahead[u] = (i0 + u + 1 < len) ? bits[base + (long long)(i0 + u + 1) * step] : 0u;
#pragma unroll
        for (int u = 0; u < SDFK_SCAN_AHEAD; ++u) {
            const int i = i0 + u;
            if (i < len) {
                const unsigned next = ahead[u];
                if (i >= 1) m ^= cur & ~prev;
                if (i + 1 < len) f ^= cur & ~next;
                pm[base + (long long)i * step] = m;
                pf[base + (long long)i * step] = f;
                prev = cur;
                cur = next;
            }
        }
    }
}
// 3. inside = (m0 | f0') & (m1 | f1'), one thread per word.
//    signed (:250-254, 261-264): f' = the cumulative sum of the falling edges, flipped — the value at the mirrored index;
//    signed_old (:185-203): fmark counts the falling edges at or after the point (a true reverse sum): total ^ prefix[i-1]
__global__ __launch_bounds__(256) void sdfk_signed_combine_kernel(const unsigned* __restrict__ m0, const unsigned* __restrict__ f0,
                                                                  const unsigned* __restrict__ m1, const unsigned* __restrict__ f1,
                                                                  unsigned* __restrict__ inside, int n0, int n1, int kw,
                                                                  int reverse_sum) {
    // one plane per blockIdx.y, its n1 x kw words flattened (kw is 17 at 513 points: a 64-wide word axis idled 3 lanes in 4)
    const unsigned r = sdfk_bx() * 256 + sdfk_tx();
    if (r >= (unsigned)(n1 * kw)) return;
    const int j = (int)(r / (unsigned)kw), w = (int)(r - (unsigned)j * kw), i = sdfk_by();
    const long long s0 = (long long)n1 * kw, s1 = kw, t = (long long)i * s0 + (long long)j * s1 + w;
    unsigned g0, g1;
    if (reverse_sum) {
        g0 = f0[t + (long long)(n0 - 1 - i) * s0] ^ (i >= 1 ? f0[t - s0] : 0u);
        g1 = f1[t + (long long)(n1 - 1 - j) * s1] ^ (j >= 1 ? f1[t - s1] : 0u);
    } else {
        g0 = f0[t + (long long)(n0 - 1 - 2 * i) * s0];
        g1 = f1[t + (long long)(n1 - 1 - 2 * j) * s1];
    }
    inside[t] = (m0[t] | g0) & (m1[t] | g1);
}
// 4. conv_averaging(inside, (2,2,1), 1) -> crop [1:-1]^3 -> pad "edge" -> sign = 1 - 2*(avg > 0.5).
// The box of 2 taps covers offsets {0, +1}; avg > 0.5 <=> at least 3 of the 4 cells are set (exact in integers):
// word-wide, a majority-of-four. The crop-and-pad is an index clamp: along i and j on the cells, along k on the bits
// (bit 0 repeats bit 1, bit n2-1 repeats bit n2-2 — which may sit in the word before). One thread per word of `flip`.
static __device__ __forceinline__ unsigned sdfk_signed_majority(const unsigned* __restrict__ inside, int n0, int n1, int kw,
                                                                int crop, int i, int j, int w) {
    // signed: interior[1:-1] padded back with its edge values; signed_old (:163-218): no crop
    const int ic = crop ? min(max(i, 1), n0 - 2) : i, jc = crop ? min(max(j, 1), n1 - 2) : j;
    const int i1 = sdfk_reflect(ic + 1, n0), j1 = sdfk_reflect(jc + 1, n1);
    const long long s0 = (long long)n1 * kw;
    const unsigned a = inside[ic * s0 + (long long)jc * kw + w], b = inside[i1 * s0 + (long long)jc * kw + w];
    const unsigned c = inside[ic * s0 + (long long)j1 * kw + w], e = inside[i1 * s0 + (long long)j1 * kw + w];
    return ((a & b) & (c | e)) | ((c & e) & (a | b));
}
__global__ __launch_bounds__(256) void sdfk_signed_flip_kernel(const unsigned* __restrict__ inside, unsigned* __restrict__ flip,
                                                               int n0, int n1, int n2, int kw, int crop) {
    const unsigned r = sdfk_bx() * 256 + sdfk_tx();
    if (r >= (unsigned)(n1 * kw)) return;
    const int j = (int)(r / (unsigned)kw), w = (int)(r - (unsigned)j * kw), i = sdfk_by();
    unsigned f = sdfk_signed_majority(inside, n0, n1, kw, crop, i, j, w);
    if (crop) {
        if (w == 0) f = (f & ~1u) | ((f >> 1) & 1u);           // k = 0 takes k = 1
        const int kl = n2 - 1, ks = n2 - 2;                    // k = n2 - 1 takes k = n2 - 2
        if (w == (kl >> 5)) {
            const unsigned src = (ks >> 5) == w ? f : sdfk_signed_majority(inside, n0, n1, kw, crop, i, j, ks >> 5);
            f = (f & ~(1u << (kl & 31))) | (((src >> (ks & 31)) & 1u) << (kl & 31));
        }
    }
    flip[((long long)i * n1 + j) * kw + w] = f;
}
// 5. s *= sign. `s` holds the planes [plane0, plane0 + planes) of the grid (the whole grid: 0, n0); `flip` always the
// whole grid. One thread per 4 consecutive k of one row (they share a flip word) and SDFK_SIGNED_PLANES planes; the
// field is touched only where it flips: outside the body whole waves skip both the load and the store.
#define SDFK_SIGNED_PLANES 8   // planes per workgroup (one point per thread was dispatch-bound)
typedef float sdfk_row4 __attribute__((ext_vector_type(4), aligned(4)));
__global__ __launch_bounds__(256) void sdfk_signed_apply_kernel(float* __restrict__ s, const unsigned* __restrict__ flip,
                                                                GridDims d, int kw, int plane0, int planes) {
    const int j = sdfk_by() * 4 + (sdfk_tx() >> 6), k = (sdfk_bx() * 64 + (sdfk_tx() & 63)) * 4;
    if (k >= d.n2 || j >= d.n1) return;
    const int lb = sdfk_bz() * SDFK_SIGNED_PLANES;
    const bool whole = k + 4 <= d.n2;
    unsigned nib[SDFK_SIGNED_PLANES];
#pragma unroll
    for (int u = 0; u < SDFK_SIGNED_PLANES; ++u)
        nib[u] = lb + u < planes ? (flip[((long long)(plane0 + lb + u) * d.n1 + j) * kw + (k >> 5)] >> (k & 31)) & 15u : 0u;
#pragma unroll
    for (int u = 0; u < SDFK_SIGNED_PLANES; ++u) {
        if (nib[u] == 0u) continue;
        float* at = s + ((long long)(lb + u) * d.n1 + j) * d.n2 + k;
        if (nib[u] == 15u && whole) {                          // (rows are only 4-byte aligned when n2 is odd)
            const sdfk_row4 v = *reinterpret_cast<const sdfk_row4*>(at);
            *reinterpret_cast<sdfk_row4*>(at) = -v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (((nib[u] >> e) & 1u) && k + e < d.n2) at[e] = -at[e];
        }
    }
}

// min over a field (sdfk_fkey + atomicMin)
__global__ __launch_bounds__(256) void sdfk_fieldmin_kernel(const float* __restrict__ s, long long n, unsigned* __restrict__ key) {
    unsigned best = 0xffffffffu;
    // NaN (tested on the bits: the library is built with -fno-honor-nans) forces "negative", so that the field is
    // returned untouched, as np.amin's NaN does in the reference
    auto take = [&](float v) {
        const unsigned u = __float_as_uint(v);
        best = (u & 0x7fffffffu) > 0x7f800000u ? 0u : min(best, sdfk_fkey(v));
    };
    const long long quads = n / 4;                             // the field is 16-byte aligned (checked by the caller)
    for (long long q = (long long)sdfk_bx() * 256 + sdfk_tx(); q < quads; q += (long long)sdfk_gx() * 256) {
        const float4 v = reinterpret_cast<const float4*>(s)[q];
        take(v.x);
        take(v.y);
        take(v.z);
        take(v.w);
    }
    if (sdfk_bx() == 0 && sdfk_tx() < n - quads * 4) take(s[quads * 4 + sdfk_tx()]);
    for (int off = 32; off > 0; off >>= 1) best = min(best, (unsigned)__shfl_down((int)best, off));
    __shared__ unsigned wave_best[4];                          // one atomic per workgroup: they serialise on one address
    if ((sdfk_tx() & 63) == 0) wave_best[sdfk_tx() >> 6] = best;
    __syncthreads();
    if (sdfk_tx() == 0) atomicMin(key, min(min(wave_best[0], wave_best[1]), min(wave_best[2], wave_best[3])));
}

static int grid_dims_ok(int64_t n0, int64_t n1, int64_t n2, GridDims* d, const char* who) {
    if (n0 < 1 || n1 < 1 || n2 < 1 || n0 > 0x3fffffff || n1 > 0x3fffffff || n2 > 0x3fffffff)
        return fail(-1, std::string(who) + ": bad grid shape");
    d->n0 = (int)n0;
    d->n1 = (int)n1;
    d->n2 = (int)n2;
    return 0;
}
static inline unsigned blocks256(long long n) { return (unsigned)((n + 255) / 256); }

extern "C" int sdfk_field_min(const float* d_field, int64_t n, float* out_min, void* stream_) {
    if (!d_field || !out_min || n < 1) return fail(-1, "sdfk_field_min: bad arguments");
    if ((uintptr_t)d_field & 15) return fail(-1, "sdfk_field_min: the field must be 16-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    unsigned* d_key = nullptr;
    HIPCHK(hipMalloc(&d_key, sizeof(unsigned)));
    const unsigned init = 0xffffffffu;
    hipError_t e = hipMemcpyAsync(d_key, &init, sizeof init, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) {
        const unsigned blocks = (unsigned)std::min<long long>((n / 4 + 255) / 256 + 1, 2048);
        hipLaunchKernelGGL(sdfk_fieldmin_kernel, dim3(blocks), dim3(256), 0, stream, d_field, (long long)n, d_key);
        e = hipGetLastError();
    }
    unsigned key = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&key, d_key, sizeof key, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFree(d_key);
    if (e != hipSuccess) return fail(-6, std::string("sdfk_field_min: ") + hipGetErrorString(e));
    const unsigned u = (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
    memcpy(out_min, &u, sizeof u);
    return 0;
}

// scratch: n0*n1*n2*4 bytes of device memory owned by the caller (NULL: allocated and freed here, which costs
// more than the operator itself on large fields)
struct Scratch {
    void* p = nullptr;
    bool own = false;
    int get(void* given, size_t bytes) {
        if (given) {
            p = given;
            return 0;
        }
        own = true;
        return hipMalloc(&p, bytes) == hipSuccess ? 0 : -1;
    }
    ~Scratch() {
        if (own && p) (void)hipFree(p);
    }
};

extern "C" int sdfk_grid_box_average(float* d_field, int64_t n0, int64_t n1, int64_t n2, int k0, int k1, int k2,
                                     int iterations, void* d_scratch, void* stream_) {
    GridDims d;
    if (!d_field) return fail(-1, "sdfk_grid_box_average: null field");
    int rc = grid_dims_ok(n0, n1, n2, &d, "sdfk_grid_box_average");
    if (rc) return rc;
    if (k0 < 1 || k1 < 1 || k2 < 1 || iterations < 0) return fail(-1, "sdfk_grid_box_average: bad kernel size / iterations");
    if (iterations == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    const long long n = (long long)n0 * n1 * n2;
    BoxVariant v;
    rc = box_variant(d, k0, k1, k2, &v);
    if (rc) return rc;
    Scratch sc;
    if (sc.get(d_scratch, (size_t)n * sizeof(float))) return fail(-5, "sdfk_grid_box_average: out of device memory");
    float* d_tmp = static_cast<float*>(sc.p);
    const double inv = 1.0 / ((double)v.k0 * v.k1 * v.k2);
    float *src = d_field, *dst = d_tmp;
    for (int it = 0; it < iterations; ++it) {
        box_launch(src, dst, v, inv, 0, stream);
        std::swap(src, dst);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && src != d_field)
        e = hipMemcpyAsync(d_field, src, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(-6, std::string("sdfk_grid_box_average: ") + hipGetErrorString(e));
    return 0;
}

extern "C" int sdfk_grid_edge_detect(float* d_field, int64_t n0, int64_t n1, int64_t n2, void* d_scratch, void* stream_) {
    GridDims d;
    if (!d_field) return fail(-1, "sdfk_grid_edge_detect: null field");
    int rc = grid_dims_ok(n0, n1, n2, &d, "sdfk_grid_edge_detect");
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const long long n = (long long)n0 * n1 * n2;
    BoxVariant v;
    rc = box_variant(d, 3, 3, 1, &v);                          // (a flat field: (1, 3, 3) on (1, n0, n1))
    if (rc) return rc;
    Scratch sc;
    if (sc.get(d_scratch, (size_t)n * sizeof(float))) return fail(-5, "sdfk_grid_edge_detect: out of device memory");
    float* d_tmp = static_cast<float*>(sc.p);
    box_launch(d_field, d_tmp, v, 1.0, 1, stream);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(d_field, d_tmp, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(-6, std::string("sdfk_grid_edge_detect: ") + hipGetErrorString(e));
    return 0;
}

// Test aid (host only, launches nothing): the variant box_launch would run for this grid and kernel.
extern "C" int sdfk_debug_box_variant(int64_t n0, int64_t n1, int64_t n2, int k0, int k1, int k2, int* out8) {
    GridDims d;
    if (!out8) return fail(-1, "sdfk_debug_box_variant: null output");
    int rc = grid_dims_ok(n0, n1, n2, &d, "sdfk_debug_box_variant");
    if (rc) return rc;
    if (k0 < 1 || k1 < 1 || k2 < 1) return fail(-1, "sdfk_debug_box_variant: bad kernel size");
    BoxVariant v;
    rc = box_variant(d, k0, k1, k2, &v);
    if (rc) return rc;
    const int out[8] = {(v.march ? 1 : 0) | (v.fast ? 2 : 0) | (v.flat ? 4 : 0), v.k0c, v.k2c, v.pc, v.chunks,
                        (int)v.grid.x, (int)v.grid.y, (int)v.grid.z};
    memcpy(out8, out, sizeof out);
    return 0;
}

static int signed_scans(const float* d_field, const unsigned char* d_mask, float* d_slab, int plane0, int planes, GridDims d,
                        float sep_min, int crop, bool check_min, void* d_scratch, hipStream_t stream);
extern "C" int sdfk_grid_signed(float* d_field, int64_t n0, int64_t n1, int64_t n2, float sep_min, int crop,
                                void* d_scratch, void* stream_) {
    GridDims d;
    if (!d_field) return fail(-1, "sdfk_grid_signed: null field");
    int rc = grid_dims_ok(n0, n1, n2, &d, "sdfk_grid_signed");
    if (rc) return rc;
    if (crop && (n0 < 3 || n1 < 3 || n2 < 3)) return fail(-1, "sdfk_grid_signed: every grid dimension must be at least 3");
    if (n0 < 2 || n1 < 2 || n2 < 2) return fail(-1, "sdfk_grid_signed: every grid dimension must be at least 2");
    return signed_scans(d_field, nullptr, d_field, 0, d.n0, d, sep_min, crop, true, d_scratch, (hipStream_t)stream_);
}

// scans + combine on the whole grid's boundary (a float field with its threshold, or a byte mask), then the sign flip
// on the planes [plane0, plane0 + planes) held in d_slab. check_min: a field with a negative value (or a NaN) is
// already signed and returned as is (C/modifications.py:236-237) — the minimum comes out of the boundary pass
static int signed_scans(const float* d_field, const unsigned char* d_mask, float* d_slab, int plane0, int planes, GridDims d,
                        float sep_min, int crop, bool check_min, void* d_scratch, hipStream_t stream) {
    const long long n0 = d.n0, n1 = d.n1, n2 = d.n2, n = n0 * n1 * n2;
    if (n0 > 65535 || n1 > 65535) return fail(-1, "sdfk_grid_signed: grid dimension beyond 65535");
    const int kw = (int)((n2 + 31) / 32);
    const long long words = n0 * n1 * kw;
    // six bit-plane arrays: boundary, (mark, falling) x 2 axes, inside; one word for the minimum. Of the caller's
    // scratch (4 bytes per point, include/sdfk.h) 3 are counted on: enough from n2 = 11 up; thinner grids get their own
    const size_t need = (size_t)(words * 6 + 4) * sizeof(unsigned);
    Scratch sc;
    if (sc.get(need <= (size_t)n * 3 ? d_scratch : nullptr, need)) return fail(-5, "sdfk_grid_signed: out of device memory");
    unsigned* bits = static_cast<unsigned*>(sc.p);
    unsigned *m0 = bits + words, *f0 = bits + 2 * words, *m1 = bits + 3 * words, *f1 = bits + 4 * words, *inside = bits + 5 * words;
    unsigned* d_key = check_min ? bits + 6 * words : nullptr;
    hipError_t e = hipSuccess;
    if (d_key) e = hipMemsetAsync(d_key, 0xff, sizeof(unsigned), stream);
    if (e != hipSuccess) return fail(-6, std::string("sdfk_grid_signed: ") + hipGetErrorString(e));
    const long long waves = (n0 * n1 + SDFK_BITS_LINES - 1) / SDFK_BITS_LINES * ((n2 + 63) / 64);
    if (waves > 0xffffffffll) return fail(-1, "sdfk_grid_signed: grid too large");
    hipLaunchKernelGGL(sdfk_signed_bits_kernel, dim3((unsigned)std::min<long long>((waves + 3) / 4, 4096)), dim3(256), 0, stream, d_field, d_mask, bits,
                       n0 * n1, (int)n2, kw, sep_min, d_key);
    if (d_key) {
        unsigned key = 0;
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&key, d_key, sizeof key, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return fail(-6, std::string("sdfk_grid_signed: ") + hipGetErrorString(e));
        if (key < 0x7fffffffu) return 0;                      // below the key of -0.0: a negative value or a NaN
    }
    // both scans in one launch: they are latency chains, not bandwidth
    const unsigned blocks0 = blocks256(n1 * kw), blocks1 = blocks256(n0 * kw);
    hipLaunchKernelGGL(sdfk_signed_scan_kernel, dim3(blocks0 + blocks1), dim3(256), 0, stream, bits, m0, f0, m1, f1, (int)n0, (int)n1,
                       kw, blocks0);
    const dim3 gridc(blocks256(n1 * kw), (unsigned)n0);
    hipLaunchKernelGGL(sdfk_signed_combine_kernel, gridc, dim3(256), 0, stream, m0, f0, m1, f1, inside, (int)n0, (int)n1, kw,
                       crop ? 0 : 1);
    if (planes > 0) {
        unsigned* flip = m0;                                   // (the scans' arrays are free again)
        hipLaunchKernelGGL(sdfk_signed_flip_kernel, gridc, dim3(256), 0, stream, inside, flip, (int)n0, (int)n1, (int)n2, kw, crop);
        const dim3 grids((unsigned)((n2 + 255) / 256), (unsigned)((n1 + 3) / 4), (unsigned)((planes + SDFK_SIGNED_PLANES - 1) / SDFK_SIGNED_PLANES));
        hipLaunchKernelGGL(sdfk_signed_apply_kernel, grids, dim3(256), 0, stream, d_slab, flip, d, kw, plane0, planes);
    }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(-6, std::string("sdfk_grid_signed: ") + hipGetErrorString(e));
    return 0;
}

// ---- `signed` on a slab of a sharded grid (aegolius_amd.distributed) ---------------------------------------------
// The scan lines of `signed` cross every slab, but all they look at is ONE BIT per point: field < min spacing. Each
// rank computes that test for its own planes (sdfk_grid_boundary_mask), the ranks exchange the bytes (1 B/point
// against the 16 B/point the evaluation moved), every rank runs the scans on the whole grid's mask and flips the sign
// of the planes it holds (sdfk_grid_signed_slab). The "already signed" test (C/modifications.py:236-237) is the
// caller's: a min over all ranks.
__global__ __launch_bounds__(256) void sdfk_boundary_mask_kernel(const float* __restrict__ s, long long n, float sep_min,
                                                                 unsigned char* __restrict__ m) {
    const long long i = ((long long)sdfk_bx() * 256 + sdfk_tx()) * 4;
    if (i + 3 < n) {
        const uchar4 v = make_uchar4(s[i] < sep_min, s[i + 1] < sep_min, s[i + 2] < sep_min, s[i + 3] < sep_min);
        m[i] = v.x; m[i + 1] = v.y; m[i + 2] = v.z; m[i + 3] = v.w;
    } else {
        for (long long t = i; t < n; ++t) m[t] = s[t] < sep_min;
    }
}
extern "C" int sdfk_grid_boundary_mask(const float* d_field, int64_t n, float sep_min, unsigned char* d_mask, void* stream_) {
    if (n < 0 || (n > 0 && (!d_field || !d_mask))) return fail(-1, "sdfk_grid_boundary_mask: bad arguments");
    if (n == 0) return 0;
    hipLaunchKernelGGL(sdfk_boundary_mask_kernel, dim3(blocks256((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream_, d_field,
                       (long long)n, sep_min, d_mask);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int sdfk_grid_signed_slab(float* d_slab, int64_t plane0, int64_t planes, const unsigned char* d_mask, int64_t n0,
                                     int64_t n1, int64_t n2, int crop, void* d_scratch, void* stream_) {
    GridDims d;
    if (!d_slab || !d_mask) return fail(-1, "sdfk_grid_signed_slab: null argument");
    int rc = grid_dims_ok(n0, n1, n2, &d, "sdfk_grid_signed_slab");
    if (rc) return rc;
    if (crop && (n0 < 3 || n1 < 3 || n2 < 3)) return fail(-1, "sdfk_grid_signed_slab: every grid dimension must be at least 3");
    if (n0 < 2 || n1 < 2 || n2 < 2) return fail(-1, "sdfk_grid_signed_slab: every grid dimension must be at least 2");
    if (plane0 < 0 || planes < 0 || plane0 + planes > n0) return fail(-1, "sdfk_grid_signed_slab: planes outside the grid");
    if (planes == 0) return 0;
    return signed_scans(nullptr, d_mask, d_slab, (int)plane0, (int)planes, d, 0.0f, crop, false, d_scratch, (hipStream_t)stream_);
}
