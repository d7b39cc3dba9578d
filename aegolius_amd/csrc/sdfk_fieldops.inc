// sdfk_fieldops.inc — consumers of a field that stays resident in HBM (included by sdfk.hip after sdfk_gridops.inc).
//
// SURVEY §8(f).3: what the reference does with the (N,) field right after create():
//   GenericGeometry.point_cloud   C/geom.py:62-74              mask = field <= 0 ; co[:2, mask]   -> sdfk_field_select
//   vector_functions.from_sdf     C/vector_functions.py:130-140  np.gradient(smarter_reshape(field)) then
//                                 batch_normalize (C/vector_modification_functions.py:14-20)       -> sdfk_field_gradient
// Both are HBM-bound: select reads the field once (4 B/point, plus 1/8 B/point of packed flags written and read back) and
// writes 8 B per selected point;
// gradient reads 4 B and writes 4 B per component and point.

#include "sdfk_vecdev.h"

// ---- ordered selection (stream compaction of indices) -------------------------------------------------------------
// A workgroup owns a tile of 8192 consecutive points: 8 rounds of 256 aligned quads. All 8 loads are issued before
// anything is counted (bytes in flight), the ranks come from 8 wave prefix sums and ONE exchange through LDS.
#define SDFK_SEL_THREADS 256
#define SDFK_SEL_ITERS 8
#define SDFK_SEL_TILE (SDFK_SEL_THREADS * 4 * SDFK_SEL_ITERS)   // points per tile
#ifndef SDFK_SEL_TPW
#define SDFK_SEL_TPW 4                                          // tiles per workgroup of the count pass
#endif

static __device__ __forceinline__ int sdfk_wave_inclusive(int v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// (selection key: sdfk_sel_key, sdfk_access.h — shared with the evaluation kernels that write flags directly)
// flags of the 4 points starting at i (bit e = field[i+e] <= threshold, as keys)
static __device__ __forceinline__ unsigned sdfk_sel_flags(const float* __restrict__ f, long long i, long long n, unsigned thr) {
    if (i + 4 <= n) {
        const sdfk_f4 v = __builtin_nontemporal_load(reinterpret_cast<const sdfk_f4*>(f + i));
        return (sdfk_sel_key(v[0]) <= thr ? 1u : 0u) | (sdfk_sel_key(v[1]) <= thr ? 2u : 0u) |
               (sdfk_sel_key(v[2]) <= thr ? 4u : 0u) | (sdfk_sel_key(v[3]) <= thr ? 8u : 0u);
    }
    unsigned m = 0;
    for (int e = 0; e < 4; ++e)
        if (i + e < n && sdfk_sel_key(f[i + e]) <= thr) m |= 1u << e;
    return m;
}

// pass 1: selected points per workgroup tile
template <bool PACK>   // PACK = false: a pure count (no flags written: a read-only stream runs ~20 % faster)
__global__ __launch_bounds__(SDFK_SEL_THREADS) void sdfk_select_count_kernel(const float* __restrict__ f, long long n, unsigned thr,
                                                                             unsigned long long* __restrict__ blk,
                                                                             unsigned* __restrict__ packed) {
    __shared__ int wsum[2][SDFK_SEL_THREADS / 64];
    // SDFK_SEL_TPW consecutive tiles per workgroup: a tile is 32 KB of field, 5 us of work — the launch of 131 K workgroups
    // of that size at 1025^3 showed in the read rate (the partial sums are double-buffered: one barrier per tile)
    // the quads of the NEXT tile are requested before this one is counted (round 4: a tile's loads used to start after the
    // barrier of the tile before it; three process pairs on one box, old / new: count pass 0.853 / 0.857, 0.867 / 0.765,
    // 0.865 / 0.785 ms at 1025^3, whole selection 1.29 / 1.24, 1.18 / 1.13, 1.29 / 1.22 — profiles/r04_select_prefetch.txt);
    // tiles that reach past n take the element-wise path as before
    sdfk_f4 nxt[SDFK_SEL_ITERS];
    auto whole = [&](long long tile) { return (tile + 1) * (long long)SDFK_SEL_TILE <= n; };
    auto request = [&](long long tile) {
        const long long base = tile * SDFK_SEL_TILE + sdfk_tx() * 4;
#pragma unroll
        for (int it = 0; it < SDFK_SEL_ITERS; ++it)
            nxt[it] = __builtin_nontemporal_load(reinterpret_cast<const sdfk_f4*>(f + base + (long long)it * SDFK_SEL_THREADS * 4));
    };
    const long long tile0 = (long long)sdfk_bx() * SDFK_SEL_TPW;
    if (whole(tile0)) request(tile0);
#pragma unroll 1
  for (int tt = 0; tt < SDFK_SEL_TPW; ++tt) {
    const long long tile = tile0 + tt;
    const long long base = tile * SDFK_SEL_TILE + sdfk_tx() * 4;
    if (tile * SDFK_SEL_TILE >= n) break;
    unsigned m[SDFK_SEL_ITERS];
    if (whole(tile)) {
        sdfk_f4 cur[SDFK_SEL_ITERS];
#pragma unroll
        for (int it = 0; it < SDFK_SEL_ITERS; ++it) cur[it] = nxt[it];
        if (tt + 1 < SDFK_SEL_TPW && whole(tile + 1)) request(tile + 1);
#pragma unroll
        for (int it = 0; it < SDFK_SEL_ITERS; ++it)
            m[it] = (sdfk_sel_key(cur[it][0]) <= thr ? 1u : 0u) | (sdfk_sel_key(cur[it][1]) <= thr ? 2u : 0u) |
                    (sdfk_sel_key(cur[it][2]) <= thr ? 4u : 0u) | (sdfk_sel_key(cur[it][3]) <= thr ? 8u : 0u);
    } else {
#pragma unroll
        for (int it = 0; it < SDFK_SEL_ITERS; ++it) {
            const long long i = base + (long long)it * SDFK_SEL_THREADS * 4;
            m[it] = i < n ? sdfk_sel_flags(f, i, n, thr) : 0u;
        }
    }
    int c = 0;
#pragma unroll
    for (int it = 0; it < SDFK_SEL_ITERS; ++it) c += __popc(m[it]);
    const int lane = sdfk_tx() & 63;
    if (PACK) {
        // the flags as a LINEAR bit string (bit j of word w = point 32 w + j: what the scatter pass of the fused selection
        // reads, one word per thread, ONE prefix sum per tile instead of one per round): in round `it` the thread's 4 flags
        // are nibble (thread % 8) of word it * 32 + thread / 8 — eight lanes make a word (three exchange steps)
#pragma unroll
        for (int it = 0; it < SDFK_SEL_ITERS; ++it) {
            unsigned w = m[it] << (4u * (unsigned)(lane & 7));
            w |= __shfl_xor(w, 1);
            w |= __shfl_xor(w, 2);
            w |= __shfl_xor(w, 4);
            if ((lane & 7) == 0) packed[tile * SDFK_SEL_THREADS + it * (SDFK_SEL_THREADS / 8) + (sdfk_tx() >> 3)] = w;
        }
    }
    c = sdfk_wave_inclusive(c, lane);
    if (lane == 63) wsum[tt & 1][sdfk_tx() >> 6] = c;
    __syncthreads();
    if (sdfk_tx() == 0) {
        int t = 0;
        for (int w = 0; w < SDFK_SEL_THREADS / 64; ++w) t += wsum[tt & 1][w];
        blk[tile] = (unsigned long long)t;
    }
  }
}

// pass 2: counts -> exclusive offsets, in place; blk[nb] = total. One workgroup walks the array in chunks of 4096
// entries (4 consecutive per thread: coalesced 32-byte loads), the next chunk's loads in flight while this one is
// scanned: wave prefix by shuffles, the 16 wave totals through LDS.
#define SDFK_SCAN_PER 4
static __device__ __forceinline__ unsigned long long sdfk_wave_inclusive64(unsigned long long v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned lo = __shfl_up((unsigned)v, d, 64), hi = __shfl_up((unsigned)(v >> 32), d, 64);
        if (lane >= d) v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}
__global__ __launch_bounds__(1024) void sdfk_select_scan_kernel(unsigned long long* __restrict__ blk, long long nb) {
    __shared__ unsigned long long wtot[2][16];
    const int lane = sdfk_tx() & 63, wave = sdfk_tx() >> 6;
    unsigned long long carry = 0, cur[SDFK_SCAN_PER], nxt[SDFK_SCAN_PER];
    const long long chunk = 1024 * SDFK_SCAN_PER;
    for (int e = 0; e < SDFK_SCAN_PER; ++e) {
        const long long i = (long long)sdfk_tx() * SDFK_SCAN_PER + e;
        cur[e] = i < nb ? blk[i] : 0;
    }
    int flip = 0;
    for (long long base = 0; base < nb; base += chunk, flip ^= 1) {
        for (int e = 0; e < SDFK_SCAN_PER; ++e) {
            const long long i = base + chunk + (long long)sdfk_tx() * SDFK_SCAN_PER + e;
            nxt[e] = i < nb ? blk[i] : 0;
        }
        unsigned long long s = 0;
        for (int e = 0; e < SDFK_SCAN_PER; ++e) s += cur[e];
        const unsigned long long incl = sdfk_wave_inclusive64(s, lane);
        if (lane == 63) wtot[flip][wave] = incl;
        __syncthreads();                                      // wtot is double-buffered: one barrier per chunk
        unsigned long long before = carry, all = 0;
        for (int w = 0; w < 16; ++w) {
            before += w < wave ? wtot[flip][w] : 0;
            all += wtot[flip][w];
        }
        unsigned long long run = before + incl - s;
        for (int e = 0; e < SDFK_SCAN_PER; ++e) {
            const long long i = base + (long long)sdfk_tx() * SDFK_SCAN_PER + e;
            if (i < nb) blk[i] = run;
            run += cur[e];
            cur[e] = nxt[e];
        }
        carry += all;
    }
    if (sdfk_tx() == 0) blk[nb] = carry;
}

// ---- fused selection: evaluate -> flags -> compact (GenericGeometry.point_cloud without a field) --------------------
// The evaluation kernels write one bit per point when they are handed a flag buffer. One 32-bit SLOT per (row, window):
// window k of row r covers the flat indices [32 (floor(r L / 32) + k), + 32) and carries the bits of the points of row r in
// it (rows of L points; a flat window shared by two rows has a slot in each). Slots are stored BRICK-TILED,
// word((r, k)) = ((r / RB) * nchunk + k) * RB + r % RB with RB = 16 for the row-block kernels (a brick's 16 words are one
// contiguous 64-byte store) and RB = 1, one row of n points, for the plain kernels (the linear bit string). Counting and
// compaction walk the slots in ROW order — (r, k) ascending is ascending flat index — in tiles of 256 slots, one per thread.
struct SelGeom {
    long long L;            // points per row
    long long R;            // rows
    unsigned nchunk;        // slots per row
    unsigned RB;            // rows per block of the tiled layout
    long long nslots;       // R * nchunk
};
static SelGeom sel_geom(long long n, long long row_len, bool tiled) {
    SelGeom g;
    if (tiled) {
        g.L = row_len;
        g.R = n / row_len;
        g.nchunk = (unsigned)((row_len % 32 == 0) ? row_len / 32 : (row_len + 62) / 32);
        g.RB = 16;
    } else {
        g.L = n;
        g.R = 1;
        g.nchunk = (unsigned)((n + 31) / 32 + 1);
        g.RB = 1;
    }
    g.nslots = g.R * (long long)g.nchunk;
    return g;
}
static long long sel_words(const SelGeom& g) {              // words of the tiled array (whole blocks)
    return ((g.R + g.RB - 1) / g.RB) * (long long)g.RB * g.nchunk;
}
static __device__ __forceinline__ unsigned sdfk_slot_word(const unsigned* __restrict__ flags, const SelGeom& g, long long slot,
                                                          long long* flat0) {
    if (slot >= g.nslots) {
        *flat0 = 0;
        return 0u;
    }
    const long long r = slot / g.nchunk;
    const unsigned k = (unsigned)(slot - r * g.nchunk);
    *flat0 = (((r * g.L) >> 5) + k) << 5;
    return flags[((r / g.RB) * g.nchunk + k) * g.RB + (r % g.RB)];
}
__global__ __launch_bounds__(SDFK_SEL_THREADS) void sdfk_flags_count_kernel(const unsigned* __restrict__ flags, SelGeom g,
                                                                            unsigned long long* __restrict__ blk) {
    __shared__ int wsum[SDFK_SEL_THREADS / 64];
    long long flat0;
    const unsigned word = sdfk_slot_word(flags, g, (long long)sdfk_bx() * SDFK_SEL_THREADS + sdfk_tx(), &flat0);
    const int c = sdfk_wave_inclusive(__popc(word), sdfk_tx() & 63);
    if ((sdfk_tx() & 63) == 63) wsum[sdfk_tx() >> 6] = c;
    __syncthreads();
    if (sdfk_tx() == 0) {
        int t = 0;
        for (int w = 0; w < SDFK_SEL_THREADS / 64; ++w) t += wsum[w];
        blk[sdfk_bx()] = (unsigned long long)t;
    }
}
// (total / capacity: when the caller enqueues the scatter BEHIND the scan without having read the count — one stream
//  synchronisation for the whole selection instead of two — the kernel itself stays out of an index buffer that is too
//  small; total == nullptr: the host has checked)
__global__ __launch_bounds__(SDFK_SEL_THREADS) void sdfk_flags_scatter_kernel(const unsigned* __restrict__ flags, SelGeom g,
                                                                              const unsigned long long* __restrict__ blk,
                                                                              long long* __restrict__ index,
                                                                              const unsigned long long* __restrict__ total_p = nullptr,
                                                                              long long capacity = 0) {
    if (total_p && (long long)*total_p > capacity) return;
    __shared__ int wsum[SDFK_SEL_THREADS / 64];
    __shared__ long long tile0;                                // flat index of the tile's first window
    __shared__ unsigned short local[SDFK_SEL_THREADS * 32];    // offsets from there: 256 slots span at most 8192 points
    const int lane = sdfk_tx() & 63, wave = sdfk_tx() >> 6;
    long long flat0;
    unsigned word = sdfk_slot_word(flags, g, (long long)sdfk_bx() * SDFK_SEL_THREADS + sdfk_tx(), &flat0);
    // (a row's slots past its last point are empty but may start up to two windows beyond the next row's first one:
    //  the offsets are taken from a little before the first slot's window, so that none of them is negative)
    if (sdfk_tx() == 0) tile0 = flat0 - 96;
    const int c = __popc(word);
    const int incl = sdfk_wave_inclusive(c, lane);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    const long long base = tile0;
    int before = 0, total = 0;
    for (int w = 0; w < SDFK_SEL_THREADS / 64; ++w) {
        before += w < wave ? wsum[w] : 0;
        total += wsum[w];
    }
    int at = before + incl - c;
    while (word) {                                             // ascending bits = ascending points
        const int bit = __builtin_ctz(word);
        word &= word - 1u;
        local[at++] = (unsigned short)(flat0 - base + bit);
    }
    __syncthreads();
    long long* dst = index + blk[sdfk_bx()];
    for (int r = sdfk_tx(); r < total; r += SDFK_SEL_THREADS) dst[r] = base + local[r];
}


// scratch layout: (nb + 1) offsets of 8 bytes, then nb * 256 words of packed flags (n / 8 bytes)
extern "C" size_t sdfk_field_select_scratch(int64_t n) {
    const long long nb = n > 0 ? (n + SDFK_SEL_TILE - 1) / SDFK_SEL_TILE : 0;
    return (size_t)(nb + 1) * sizeof(unsigned long long) + (size_t)nb * SDFK_SEL_THREADS * sizeof(unsigned);
}

// pass 3: the indices from the linear flag words (the scatter kernel of the fused selection: one word per thread)
static int select_scatter(long long nb, unsigned long long* blk, int64_t* d_index, hipStream_t stream) {
    const unsigned* packed = reinterpret_cast<const unsigned*>(blk + nb + 1);
    SelGeom g;
    g.L = nb * (long long)SDFK_SEL_TILE;                       // one row: slot k = points [32 k, 32 k + 32)
    g.R = 1;
    g.nchunk = (unsigned)(nb * SDFK_SEL_THREADS);
    g.RB = 1;
    g.nslots = nb * (long long)SDFK_SEL_THREADS;
    hipLaunchKernelGGL(sdfk_flags_scatter_kernel, dim3((unsigned)nb), dim3(SDFK_SEL_THREADS), 0, stream, packed, g, blk,
                       reinterpret_cast<long long*>(d_index));
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(-6, std::string("sdfk_field_select: ") + hipGetErrorString(e));
    return 0;
}

extern "C" int sdfk_field_select(const float* d_field, int64_t n, float threshold, int64_t* d_index, int64_t capacity,
                                 int64_t* count, void* d_scratch, void* stream_) {
    if (!count || n < 0 || (n > 0 && !d_field) || capacity < 0) return fail(-1, "sdfk_field_select: bad arguments");
    if ((uintptr_t)d_field & 15) return fail(-1, "sdfk_field_select: the field must be 16-byte aligned");
    if ((uintptr_t)d_scratch & 7) return fail(-1, "sdfk_field_select: the scratch must be 8-byte aligned");
    *count = 0;
    if (n == 0) return 0;
    const unsigned thr = sdfk_sel_key(threshold);
    if (thr == 0xffffffffu) return 0;                          // NaN threshold: nothing compares <= NaN
    hipStream_t stream = (hipStream_t)stream_;
    const long long nb = (n + SDFK_SEL_TILE - 1) / SDFK_SEL_TILE;
    if (nb > 0x7fffffff) return fail(-1, "sdfk_field_select: field too large");
    Scratch sc;
    const size_t need = (d_index || d_scratch) ? sdfk_field_select_scratch(n) : (size_t)(nb + 1) * sizeof(unsigned long long);
    if (sc.get(d_scratch, need)) return fail(-5, "sdfk_field_select: out of device memory");
    unsigned long long* blk = static_cast<unsigned long long*>(sc.p);
    // flags are kept only where a scatter can follow: with an index buffer, or with a caller-owned scratch (select_finish)
    if (d_index || d_scratch)
        hipLaunchKernelGGL(sdfk_select_count_kernel<true>, dim3((unsigned)((nb + SDFK_SEL_TPW - 1) / SDFK_SEL_TPW)), dim3(SDFK_SEL_THREADS), 0, stream, d_field,
                           (long long)n, thr, blk, reinterpret_cast<unsigned*>(blk + nb + 1));
    else
        hipLaunchKernelGGL(sdfk_select_count_kernel<false>, dim3((unsigned)((nb + SDFK_SEL_TPW - 1) / SDFK_SEL_TPW)), dim3(SDFK_SEL_THREADS), 0, stream, d_field,
                           (long long)n, thr, blk, static_cast<unsigned*>(nullptr));
    hipLaunchKernelGGL(sdfk_select_scan_kernel, dim3(1), dim3(1024), 0, stream, blk, nb);
    hipError_t e = hipGetLastError();
    unsigned long long total = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&total, blk + nb, sizeof total, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(-6, std::string("sdfk_field_select: ") + hipGetErrorString(e));
    *count = (int64_t)total;
    if (!d_index || total == 0) return 0;                     // count only: the scratch keeps what select_finish needs
    if ((int64_t)total > capacity) return fail(-1, "sdfk_field_select: index buffer smaller than the selection");
    return select_scatter(nb, blk, d_index, stream);
}

// Second half of a selection whose count-only call (d_index == NULL, caller-owned d_scratch) has just run on a field
// of n points: writes the `count` indices it announced, without reading the field again.
extern "C" int sdfk_field_select_finish(int64_t n, int64_t count, int64_t* d_index, int64_t capacity, void* d_scratch,
                                        void* stream_) {
    if (n < 0 || count < 0 || capacity < 0 || !d_scratch || ((uintptr_t)d_scratch & 7))
        return fail(-1, "sdfk_field_select_finish: bad arguments");
    if (n == 0 || count == 0) return 0;
    if (!d_index || count > capacity) return fail(-1, "sdfk_field_select_finish: index buffer smaller than the selection");
    const long long nb = (n + SDFK_SEL_TILE - 1) / SDFK_SEL_TILE;
    unsigned long long* blk = static_cast<unsigned long long*>(d_scratch);
    unsigned long long total = 0;
    HIPCHK(hipMemcpy(&total, blk + nb, sizeof total, hipMemcpyDeviceToHost));
    if ((int64_t)total != count) return fail(-1, "sdfk_field_select_finish: the scratch does not hold a selection of that size");
    return select_scatter(nb, blk, d_index, (hipStream_t)stream_);
}

// ---- fused selection: host side (the slot geometry and the flag kernels are defined above, next to the field selection) ----
// scratch of the fused selection: (tiles + 1) offsets of 8 bytes, then the slot words. Sized for either layout of n points.
static long long sel_tiles(const SelGeom& g) { return (g.nslots + SDFK_SEL_THREADS - 1) / SDFK_SEL_THREADS; }
extern "C" size_t sdfk_eval_select_scratch(int64_t n, int64_t row_len) {
    if (n <= 0) return 16;
    long long words = sel_words(sel_geom(n, 0, false));         // the linear layout of the plain kernels ...
    if (row_len >= 32 && n % row_len == 0) words = std::max(words, sel_words(sel_geom(n, row_len, true)));   // ... or the tiled one
    const long long tiles = words / SDFK_SEL_THREADS + 2;
    return (size_t)(tiles + 1) * sizeof(unsigned long long) + (size_t)(words + 128) * sizeof(unsigned);
}
struct SelScratch {
    unsigned long long* blk;
    unsigned* flags;
    long long tiles;
};
static SelScratch sel_scratch(void* d_scratch, const SelGeom& g) {
    SelScratch sc;
    sc.tiles = sel_tiles(g);
    sc.blk = static_cast<unsigned long long*>(d_scratch);
    sc.flags = reinterpret_cast<unsigned*>(sc.blk + sc.tiles + 1);
    return sc;
}
// after the evaluation has written the flags: count, scan, (optionally) scatter
static int flags_finish(const SelGeom& g, const SelScratch& sc, int64_t* d_index, int64_t capacity, int64_t* count,
                        hipStream_t stream) {
    hipLaunchKernelGGL(sdfk_flags_count_kernel, dim3((unsigned)sc.tiles), dim3(SDFK_SEL_THREADS), 0, stream, sc.flags, g, sc.blk);
    hipLaunchKernelGGL(sdfk_select_scan_kernel, dim3(1), dim3(1024), 0, stream, sc.blk, sc.tiles);
    // with an index buffer the scatter goes right behind the scan (it checks the capacity itself, on the device) and the
    // count comes back with it: ONE synchronisation per selection (round 3: count -> sync -> scatter -> sync)
    if (d_index && capacity > 0)
        hipLaunchKernelGGL(sdfk_flags_scatter_kernel, dim3((unsigned)sc.tiles), dim3(SDFK_SEL_THREADS), 0, stream, sc.flags, g, sc.blk,
                           reinterpret_cast<long long*>(d_index), sc.blk + sc.tiles, (long long)capacity);
    hipError_t e = hipGetLastError();
    unsigned long long total = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&total, sc.blk + sc.tiles, sizeof total, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(-6, std::string("sdfk_eval_select: ") + hipGetErrorString(e));
    *count = (int64_t)total;
    if (!d_index || total == 0) return 0;
    if ((int64_t)total > capacity) return fail(-1, "sdfk_eval_select: index buffer smaller than the selection");
    return 0;
}
// Plans the evaluation of a fused selection and lays its flag words out from that plan: the row-block kernels write the
// tiled layout, the plain kernels the linear one — the kernel that writes the flags and the code that reads them take the
// layout from this one plan. row_len: the rows of the tiled layout (an array's hint, a grid's rows). On return c->plan,
// c->d_flags and c->thr_key are set and the words the kernels do not write are cleared.
static int select_prepare(EvalCall* c, EvalPlan* pl, long long row_len, float threshold, void* d_scratch, SelGeom* g, SelScratch* sc) {
    if (!d_scratch || ((uintptr_t)d_scratch & 7)) return fail(-1, "sdfk_eval_select: the scratch must be 8-byte aligned device memory");
    c->d_flags = static_cast<unsigned*>(d_scratch);            // (the planner asks whether flags are written; where follows from the plan)
    const int rc = plan_eval(*c, plan_env(), pl);
    if (rc) return rc;
    *g = sel_geom(c->n, row_len, pl->rows());
    *sc = sel_scratch(d_scratch, *g);
    c->plan = pl;
    c->d_flags = sc->flags;
    c->thr_key = sdfk_sel_key(threshold);
    hipStream_t stream = (hipStream_t)c->stream;
    // Linear layout (plain kernels): single points OR their bits in (tails, unaligned arrays), so the words start from zero.
    // Tiled layout (row-block kernels): every slot word of every block is written by exactly one brick — rows past the end
    // of the last block as zeros —, so only the padding behind the last block is cleared (round 3 cleared all n / 8 bytes:
    // 135 MB at 1025^3 in front of every selection).
    if (g->RB == 16) HIPCHK(hipMemsetAsync(sc->flags + sel_words(*g), 0, 64 * sizeof(unsigned), stream));
    else HIPCHK(hipMemsetAsync(sc->flags, 0, (size_t)(sel_words(*g) + 64) * sizeof(unsigned), stream));
    return 0;
}
// the evaluation writes the flags, then count, scan, (optionally) scatter
static int select_run(const EvalCall& c, const SelGeom& g, const SelScratch& sc, int64_t* d_index, int64_t capacity, int64_t* count) {
    hipStream_t stream = (hipStream_t)c.stream;
    if (c.thr_key == 0xffffffffu) {                            // NaN threshold: nothing compares <= NaN
        HIPCHK(hipMemsetAsync(sc.blk, 0, (size_t)(sc.tiles + 1) * sizeof(unsigned long long), stream));
        HIPCHK(hipStreamSynchronize(stream));
        return 0;
    }
    const int rc = run(c);
    if (rc) return rc;
    return flags_finish(g, sc, d_index, capacity, count, stream);
}

extern "C" int sdfk_eval_device_select(sdfk_program* p, const float* d_co, int64_t n, int64_t row_stride, int64_t row_len,
                                       int flat, float threshold, int64_t* d_index, int64_t capacity, int64_t* count,
                                       void* d_scratch, void* stream_, int mode) {
    if (!p || !d_co || !count || n < 0 || capacity < 0) return fail(-1, "sdfk_eval_device_select: bad arguments");
    if (row_stride < n) return fail(-1, "sdfk_eval_device_select: row stride smaller than the point count");
    if (row_len < 0 || (row_len > 0 && n % row_len != 0)) return fail(-1, "sdfk_eval_device_select: the point count is not a multiple of the row length");
    if (p->n_aux > 0) return fail(-1, "sdfk_eval_device_select: staged programs (auxiliary fields) are evaluated to a field first");
    *count = 0;
    if (n == 0) return 0;
    SrcArray a = {d_co, (long long)row_stride};
    EvalCall c = array_call(p, &a, n, nullptr, stream_, mode, aligned16(d_co) && (row_stride % 4 == 0));
    c.row_len = row_len;
    c.flat = flat != 0;
    EvalPlan pl;
    SelGeom g;
    SelScratch sc;
    const int rc = select_prepare(&c, &pl, row_len, threshold, d_scratch, &g, &sc);
    if (rc) return rc;
    return select_run(c, g, sc, d_index, capacity, count);
}

extern "C" int sdfk_eval_grid_select(sdfk_program* p, const float* ax0, int64_t n0, const float* ax1, int64_t n1,
                                     const float* ax2, int64_t n2, int64_t start, int64_t n, float threshold,
                                     int64_t* d_index, int64_t capacity, int64_t* count, void* d_scratch, void* stream_,
                                     int mode) {
    if (!p || !count || capacity < 0) return fail(-1, "sdfk_eval_grid_select: bad arguments");
    if (start < 0 || n < 0 || start + n > n0 * n1 * n2) return fail(-1, "sdfk_eval_grid_select: range outside the grid");
    if (p->n_aux > 0) return fail(-1, "sdfk_eval_grid_select: staged programs (auxiliary fields) are evaluated to a field first");
    *count = 0;
    if (n == 0) return 0;
    AxisTables t;
    SrcGrid sg;
    int rc = upload_axes(ax0, n0, ax1, n1, ax2, n2, (hipStream_t)stream_, &t, &sg, start);
    if (rc) return rc;
    EvalCall c = grid_call(p, &sg, n, nullptr, stream_, mode, true);
    EvalPlan pl;
    SelGeom g;
    SelScratch sc;
    rc = select_prepare(&c, &pl, n2 > 1 ? n2 : n1, threshold, d_scratch, &g, &sc);
    if (rc) return rc;
    return select_run(c, g, sc, d_index, capacity, count);     // (synchronises: the axis tables go)
}

// Second half of a fused selection whose count-only call (d_index == NULL) has just run with the same arguments: the
// indices, from the flags. There are no coordinates here: the layout is that of the plan of the same (n, row_len, mode).
extern "C" int sdfk_eval_select_finish(sdfk_program* p, int64_t n, int64_t row_len, int mode, int64_t count, int64_t* d_index,
                                       int64_t capacity, void* d_scratch, void* stream_) {
    if (!p || n < 0 || count < 0 || capacity < 0 || !d_scratch || ((uintptr_t)d_scratch & 7))
        return fail(-1, "sdfk_eval_select_finish: bad arguments");
    if (n == 0 || count == 0) return 0;
    if (!d_index || count > capacity) return fail(-1, "sdfk_eval_select_finish: index buffer smaller than the selection");
    const SrcArray a = {nullptr, 0};
    EvalCall c = array_call(p, &a, n, nullptr, stream_, mode, false);
    c.row_len = row_len;
    c.d_flags = static_cast<unsigned*>(d_scratch);
    EvalPlan pl;
    const int rc = plan_eval(c, plan_env(), &pl);
    if (rc) return rc;
    const SelGeom g = sel_geom(n, row_len, pl.rows());
    const SelScratch sc = sel_scratch(d_scratch, g);
    unsigned long long total = 0;
    HIPCHK(hipMemcpy(&total, sc.blk + sc.tiles, sizeof total, hipMemcpyDeviceToHost));
    if ((int64_t)total != count) return fail(-1, "sdfk_eval_select_finish: the scratch does not hold a selection of that size");
    hipLaunchKernelGGL(sdfk_flags_scatter_kernel, dim3((unsigned)sc.tiles), dim3(SDFK_SEL_THREADS), 0, (hipStream_t)stream_,
                       sc.flags, g, sc.blk, reinterpret_cast<long long*>(d_index));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize((hipStream_t)stream_));
    return 0;
}

// ---- gradient direction --------------------------------------------------------------------------------------------
// np.gradient with unit spacing and edge_order 1: central differences inside, one-sided first differences on the
// two faces of each axis; then every vector is divided by its Euclidean norm unless that norm is zero.
// fp32 arithmetic: a difference of two fp32 values rounded to fp32 is what the float64 difference rounds to, so
// the raw gradient equals numpy's rounded to fp32; the norm is taken after scaling by a power of two (no overflow,
// no underflow, subnormal differences keep every bit) with v_rsq_f32 (1 ulp): components within ~2e-7 of the
// float64 result. (A float64 version of this
// kernel was bound by its divisions and square root — 2.2 ms of the 4.4 at 1025^3.)
// Layout: every thread owns one 16-byte-aligned quad of the FLAT field, so the three component stores are full
// aligned lines for any grid shape; the j and i neighbours are unaligned dwordx4 loads that hit lines the same XCD
// fetched a moment ago: workgroups are numbered so that one XCD sweeps the planes i of one BAND of rows before the
// next band (the hardware deals consecutive workgroups round-robin to the 8 XCDs, hence the remap).
#define SDFK_GRAD_BAND 32         // rows per band (more when rows are short)

// difference across `pos` WITHOUT the 1/2 of the central form; *central says whether that 1/2 is still owed
static __device__ __forceinline__ float sdfk_diff(float lo, float c, float hi, int pos, int n, bool* central) {
    *central = pos != 0 && pos != n - 1;
    return pos == 0 ? hi - c : (pos == n - 1 ? c - lo : hi - lo);
}
// four values starting at q, or zeros where q + e falls outside [0, n)
static __device__ __forceinline__ void sdfk_grad_fetch(const float* __restrict__ f, long long q, long long n, float* v) {
    if (q >= 0 && q + 4 <= n) {
        const sdfk_f4u t = *reinterpret_cast<const sdfk_f4u*>(f + q);
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    } else {
        for (int e = 0; e < 4; ++e) v[e] = (q + e >= 0 && q + e < n) ? f[q + e] : 0.0f;
    }
}

__global__ __launch_bounds__(256) void sdfk_gradient_kernel(const float* __restrict__ f, GridDims d, float* __restrict__ out,
                                                            long long stride, long long n, int ncomp, int normalize, int band,
                                                            unsigned S, unsigned total) {
    const unsigned per = (total + 7) / 8;
    const unsigned L = (sdfk_bx() % 8) * per + sdfk_bx() / 8;
    if (L >= total) return;
    const unsigned s = L % S, t = L / S, i = t % (unsigned)d.n0, b = t / (unsigned)d.n0;
    const long long plane = (long long)d.n1 * d.n2;
    const long long jlo = (long long)b * band, jhi = jlo + band < d.n1 ? jlo + band : d.n1;
    const long long lo = ((long long)i * d.n1 + jlo) * d.n2, hi = ((long long)i * d.n1 + jhi) * d.n2;
    const long long p = ((lo + 3) & ~3ll) + ((long long)s * 256 + sdfk_tx()) * 4;
    if (p >= ((hi + 3) & ~3ll) || p >= n) return;
    long long q = p - (long long)i * plane;                     // position inside plane ii (a quad may start in the next one)
    int ii = (int)i;
    if (q >= plane) {
        q -= plane;
        ++ii;
    }
    int j = plane <= 0xffffffffll ? (int)((unsigned)q / (unsigned)d.n2) : (int)(q / d.n2);
    int k = (int)(q - (long long)j * d.n2);
    float c[4], zl, zr, ylo[4], yhi[4], xlo[4], xhi[4];
    sdfk_grad_fetch(f, p, n, c);
    zl = p > 0 ? f[p - 1] : 0.0f;
    zr = p + 4 < n ? f[p + 4] : 0.0f;
    if (ncomp > 1) {
        sdfk_grad_fetch(f, p - d.n2, n, ylo);
        sdfk_grad_fetch(f, p + d.n2, n, yhi);
    }
    if (ncomp > 2) {
        sdfk_grad_fetch(f, p - plane, n, xlo);
        sdfk_grad_fetch(f, p + plane, n, xhi);
    }
    sdfk_f4 o[3];
    for (int e = 0; e < 4; ++e) {
        bool cx = false, cy = false, cz;
        float gx = ncomp > 2 ? sdfk_diff(xlo[e], c[e], xhi[e], ii, d.n0, &cx) : 0.0f;
        float gy = ncomp > 1 ? sdfk_diff(ylo[e], c[e], yhi[e], j, d.n1, &cy) : 0.0f;
        float gz = sdfk_diff(e ? c[e - 1] : zl, c[e], e < 3 ? c[e + 1] : zr, k, d.n2, &cz);
        if (normalize) {
            sdfk_unit3(gx, gy, gz, cx, cy, cz);
        } else {
            gx = cx ? 0.5f * gx : gx;
            gy = cy ? 0.5f * gy : gy;
            gz = cz ? 0.5f * gz : gz;
        }
        o[0][e] = gx;
        o[1][e] = gy;
        o[2][e] = gz;
        if (++k == d.n2) {
            k = 0;
            if (++j == d.n1) {
                j = 0;
                ++ii;
            }
        }
    }
    for (int a = 3 - ncomp; a < 3; ++a) {
        float* dst = out + (long long)(a - (3 - ncomp)) * stride + p;
        if (p + 4 <= n) {
            __builtin_nontemporal_store(o[a], reinterpret_cast<sdfk_f4*>(dst));
        } else {
            for (int e = 0; p + e < n; ++e) dst[e] = o[a][e];
        }
    }
}

// ---- 3-D variant that carries the plane neighbours in registers ------------------------------------------------------
// A thread owns one 16-byte-aligned quad of the FLAT field per plane and walks SDFK_GC_SEG planes: the quad of plane
// i + 1 is the one at flat + (plane - s), s = plane mod 4, so it is aligned again — in plane coordinates the thread's
// window drifts left by s points per plane. The values of planes i - 1 and i + 1 at the window of plane i are then the
// thread's own previous / next quad shifted by s: 4 - s of them in its own registers, s in the neighbouring lane's
// (one shuffle each). The first and the last lane of a wave are halo lanes — they load and lend, they do not store — so
// there are no edge loads: a wave yields 62 quads. Per quad and plane: ONE aligned load for the next plane and the two
// unaligned row-neighbour loads, against five loads before; z neighbours come from the adjacent lanes too.
// Stores are whole aligned lines as before; quads that straddle a plane edge are written element-wise by the two
// steps that own their elements. Same arithmetic as sdfk_gradient_kernel: bit-identical results.
// Planes per thread (+ one halo plane at either end). Round 2 chose 32 (3.7 ms at 1025^3 in the process it was tuned in);
// round 4 found that this was the FAST one of the process states this kernel has on the pool's boxes and that a long walk
// is what makes the other states slow: in one process each, 32 / 8 / 4 / 3 / 2 / 1 planes take 4.34 / 4.16 / 3.73 / 3.61 /
// 3.53 / 3.81 ms in a slow process and 3.31 / - / 3.21 / 3.15 / 3.20 / 3.65 in a fast one (profiles/r04_gradient_segments.txt;
// 513^3: 0.57 -> 0.44 ms, 257^3: 0.081 -> 0.059) — two planes read the field twice (20 B/point instead of 16.5) and are
// still the fastest everywhere: the threads of a workgroup stay within a few planes of one another.
#define SDFK_GC_SEG 2
#define SDFK_GC_USE 62           // quads a wave produces

template <int S4, bool NORM>
__global__ __launch_bounds__(256) void sdfk_gradient_carry_kernel(const float* __restrict__ f, GridDims d, float* __restrict__ out,
                                                                  long long stride, long long n, unsigned wgs_per_seg,
                                                                  unsigned total, int seg_len, unsigned group) {
    // workgroups go round-robin to the 8 XCDs. group == 0: one XCD takes one contiguous eighth of the work (row
    // neighbours hit its L2, but the XCDs walk eight segments far apart: 32 regions of DRAM live at a time);
    // group > 0: an XCD takes runs of `group` consecutive chunks and all of them walk the same segment together
    unsigned L;
    if (group == 0) {
        const unsigned per = (total + 7) / 8;
        L = (sdfk_bx() % 8) * per + sdfk_bx() / 8;
    } else {
        const unsigned x = sdfk_bx() % 8, t = sdfk_bx() / 8;
        L = ((t / group) * 8 + x) * group + t % group;
    }
    if (L >= total) return;
    const unsigned seg = L / wgs_per_seg, chunk = L - seg * wgs_per_seg;
    const int lane = sdfk_tx() & 63, wave = sdfk_tx() >> 6;
    const long long plane = (long long)d.n1 * d.n2;
    const int i0 = (int)seg * seg_len, i1 = min(i0 + seg_len, d.n0);
    // quad index g: window of plane i0 starts at q = 4 g + a0, a0 such that the flat address is aligned; g from -1
    const int a0 = (int)((4 - ((long long)i0 * plane) % 4) % 4);
    const long long g = -1 + (long long)(chunk * 4u + wave) * SDFK_GC_USE + (lane - 1);
    long long q = 4 * g + a0;                                  // plane-local position of element 0 at plane i
    long long P = (long long)i0 * plane + q;                   // flat (16-byte aligned)
    // (j, k) of element 0; floor division for the windows left of the plane
    long long jq = q >= 0 ? q / d.n2 : -((-q + d.n2 - 1) / d.n2);
    int j0 = (int)jq, k0 = (int)(q - jq * d.n2);
    const bool lender = lane == 0 || lane == 63;
    float behind[4] = {0.0f, 0.0f, 0.0f, 0.0f}, centre[4], ahead[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (i0 > 0) sdfk_grad_fetch(f, P - (plane - S4), n, behind);
    sdfk_grad_fetch(f, P, n, centre);
    for (int i = i0; i < i1; ++i) {
        if (i + 1 < d.n0) sdfk_grad_fetch(f, P + (plane - S4), n, ahead);
        float ylo[4], yhi[4];
        sdfk_grad_fetch(f, P - d.n2, n, ylo);
        sdfk_grad_fetch(f, P + d.n2, n, yhi);
        // plane neighbours at this window: own quad shifted by S4, the rest from the next / previous lane
        float xlo[4], xhi[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e + S4 <= 3) xhi[e] = ahead[e + S4];
            if (e - S4 >= 0) xlo[e] = behind[e - S4];
        }
#pragma unroll
        for (int t = 0; t < S4; ++t) {
            xhi[4 - S4 + t] = __shfl_down(ahead[t], 1);         // element 4 - S4 + t  <-  next lane's ahead[t]
            xlo[t] = __shfl_up(behind[4 - S4 + t], 1);           // element t           <-  previous lane's behind[4 - S4 + t]
        }
        const float zl = __shfl_up(centre[3], 1), zr = __shfl_down(centre[0], 1);
        if (!lender) {
            sdfk_f4 o[3];
            bool valid[4];
            int j = j0, k = k0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                valid[e] = j >= 0 && j < d.n1;
                bool cx, cy, cz;
                float gx = sdfk_diff(xlo[e], centre[e], xhi[e], i, d.n0, &cx);
                float gy = sdfk_diff(ylo[e], centre[e], yhi[e], j, d.n1, &cy);
                float gz = sdfk_diff(e ? centre[e - 1] : zl, centre[e], e < 3 ? centre[e + 1] : zr, k, d.n2, &cz);
                if (NORM) {
                    sdfk_unit3(gx, gy, gz, cx, cy, cz);
                } else {
                    gx = cx ? 0.5f * gx : gx;
                    gy = cy ? 0.5f * gy : gy;
                    gz = cz ? 0.5f * gz : gz;
                }
                o[0][e] = gx;
                o[1][e] = gy;
                o[2][e] = gz;
                if (++k == d.n2) {
                    k = 0;
                    ++j;
                }
            }
            if (valid[0] || valid[3]) {
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    float* dst = out + (long long)a * stride + P;
                    if (valid[0] && valid[3]) {
                        __builtin_nontemporal_store(o[a], reinterpret_cast<sdfk_f4*>(dst));
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (valid[e]) dst[e] = o[a][e];
                    }
                }
            }
        }
        // next plane: the window moves S4 points to the left
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            behind[e] = centre[e];
            centre[e] = ahead[e];
        }
        P += plane - S4;
        k0 -= S4;
        if (k0 < 0) {
            k0 += d.n2;
            --j0;
        }
    }
}

template <int S4>
static void gradient_carry_launch(const float* f, GridDims d, float* out, long long stride, long long n, int normalize,
                                  unsigned wgs_per_seg, unsigned total, int seg_len, unsigned group, hipStream_t stream) {
    // (with groups the last round of 8 x group workgroups is filled up: indices beyond `total` leave at once)
    const dim3 grid(group ? (total + 8 * group - 1) / (8 * group) * (8 * group) : (total + 7) / 8 * 8);
    if (normalize)
        hipLaunchKernelGGL((sdfk_gradient_carry_kernel<S4, true>), grid, dim3(256), 0, stream, f, d, out, stride, n, wgs_per_seg, total, seg_len, group);
    else
        hipLaunchKernelGGL((sdfk_gradient_carry_kernel<S4, false>), grid, dim3(256), 0, stream, f, d, out, stride, n, wgs_per_seg, total, seg_len, group);
}

extern "C" int sdfk_field_gradient(const float* d_field, int64_t n0, int64_t n1, int64_t n2, int ncomp, int normalize,
                                   float* d_vec, int64_t row_stride, void* stream_) {
    GridDims d;
    if (!d_field || !d_vec) return fail(-1, "sdfk_field_gradient: null pointer");
    int rc = grid_dims_ok(n0, n1, n2, &d, "sdfk_field_gradient");
    if (rc) return rc;
    if (ncomp < 1 || ncomp > 3) return fail(-1, "sdfk_field_gradient: ncomp must be 1, 2 or 3");
    const int64_t dims[3] = {n0, n1, n2};
    for (int a = 0; a < 3; ++a) {
        if (a >= 3 - ncomp && dims[a] < 2)                    // numpy.gradient raises the same complaint
            return fail(-1, "sdfk_field_gradient: every differentiated axis needs at least 2 points");
        if (a < 3 - ncomp && dims[a] != 1) return fail(-1, "sdfk_field_gradient: axes that are not differentiated must have length 1");
    }
    const long long n = (long long)n0 * n1 * n2;
    if (row_stride < n) return fail(-1, "sdfk_field_gradient: row stride smaller than the point count");
    if (((uintptr_t)d_field & 15) || ((uintptr_t)d_vec & 15) || (row_stride & 3))
        return fail(-1, "sdfk_field_gradient: field, output and row stride must be 16-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    if (ncomp == 3 && n2 >= 8 && n0 >= 2 && !getenv("SDFK_GRADIENT_FLAT")) {
        // register-carry variant: windows from one quad left of the plane to where the last plane of a segment still
        // reaches its end (the window drifts (planes - 1) * s to the left)
        const long long plane = n1 * n2;
        const int s4 = (int)(plane % 4);
        int seg_len = SDFK_GC_SEG;
        if (const char* e = getenv("SDFK_GC_SEG")) seg_len = std::max(1, atoi(e));             // experiments
        unsigned group = 8;                                       // runs of 8 chunks per XCD (tools/grad_ab.py: 0, 1 .. 128)
        if (const char* e = getenv("SDFK_GC_GROUP")) group = (unsigned)std::max(0, atoi(e));
        const long long quads = (plane + (long long)(seg_len - 1) * s4 + 3) / 4 + 2;      // g = -1 .. quads - 2
        const long long wgs_per_seg = (quads + 4 * SDFK_GC_USE - 1) / (4 * SDFK_GC_USE);
        const long long nseg = (n0 + seg_len - 1) / seg_len, total = wgs_per_seg * nseg;
        if (total <= 0x7ffffff0ll) {
            const unsigned w = (unsigned)wgs_per_seg, t = (unsigned)total;
            switch (s4) {
                case 0: gradient_carry_launch<0>(d_field, d, d_vec, (long long)row_stride, n, normalize, w, t, seg_len, group, stream); break;
                case 1: gradient_carry_launch<1>(d_field, d, d_vec, (long long)row_stride, n, normalize, w, t, seg_len, group, stream); break;
                case 2: gradient_carry_launch<2>(d_field, d, d_vec, (long long)row_stride, n, normalize, w, t, seg_len, group, stream); break;
                default: gradient_carry_launch<3>(d_field, d, d_vec, (long long)row_stride, n, normalize, w, t, seg_len, group, stream); break;
            }
            hipError_t e = hipGetLastError();
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
            if (e != hipSuccess) return fail(-6, std::string("sdfk_field_gradient: ") + hipGetErrorString(e));
            return 0;
        }
    }
    // bands of at least 8192 points, so that a band-plane fills its workgroups
    long long band = std::max<long long>(SDFK_GRAD_BAND, (8192 + n2 - 1) / n2);
    band = std::min<long long>(band, n1);
    const long long nb = (n1 + band - 1) / band;
    const long long S = (band * n2 + 4 + 1023) / 1024, total = S * n0 * nb;
    if (total > 0x7ffffff0ll) return fail(-1, "sdfk_field_gradient: grid too large");
    hipLaunchKernelGGL(sdfk_gradient_kernel, dim3((unsigned)((total + 7) / 8 * 8)), dim3(256), 0, stream, d_field, d, d_vec,
                       (long long)row_stride, n, ncomp, normalize, (int)band, (unsigned)S, (unsigned)total);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(-6, std::string("sdfk_field_gradient: ") + hipGetErrorString(e));
    return 0;
}
