// sdfk_topology.inc — connected components, cell counts and label fields of the inside (or outside) points of a grid
// (included by sdfk.hip after sdfk_slices.inc: it uses MeshGeom, MeshSrc, mesh_eval_bits, the bit helpers of sdfk_mesh.inc
// and the tile scan of sdfk_fieldops.inc).
//
// Output definition: aegolius_amd/topology.py, include/sdfk.h and DESIGN §4.23. A point is inside by the mesh's rule
// (sdfk_sel_key(f) <= sdfk_sel_key(level), NaN outside); the region is the inside points or all the others; two points of
// the region are joined when they are grid neighbours (faces: 4 / 6, full: 8 / 26). A component's name is the smallest
// linear index among its points, components are numbered by ascending name: nothing depends on scheduling.
//
// Input: the linear bit string (32 points per word, tiles of 8192 points, zeros past n). Union-find by label equivalence,
// every phase its own launch (a kernel boundary is the only barrier there is):
//   region    the inside bits, or their complement (outside), under the valid-point mask: the evaluation is not repeated
//   init      label[p] = first point of p's row run (a maximal stretch of set bits within one grid row): bit tricks in
//             the word, a backward look over the previous words' BITS for a run that enters the word; -1 off the region
//   merge     per word and backward neighbour row: the neighbour row's bits by funnel shift, one union per stretch of
//             touching bits. The union is lock-free: roots by chasing strictly decreasing labels (relaxed agent-scope
//             loads), atomicMin of the smaller root onto the larger, retry from the returned value when that was no root
//   compress  label[p] = root of p: the component's name
//   number    root flags per word (label[p] == p), per-tile counts, the tile scan, labels rewritten to ids in place: the
//             id of root r is tile offset + word prefix + popcount of the root flags below r — 8 bytes per word of
//             scratch, no second n-word array
//   reduce    (finishing call) per row run: size by 64-bit add, box by min / max, border by or — integer atomics only,
//             so every record is order-independent; a wave whose runs all belong to one component adds once
//   moments   (its own call, from the labels alone) per row run the sums of 1, i_a, i_a i_b in closed form, 64-bit adds
//   cells     vertices, edges, squares and cubes of the cubical complex from shifted ANDs of the bit string
// No lane ever waits for another lane's write. Every loop ends by monotonic decrease and carries an iteration cap that
// raises the device error word (TOPO_ERR_*) instead of spinning: the host then fails the call.

#define SDFK_TOPO_THREADS SDFK_MESH_THREADS       // words per tile
#define TOPO_ERR_CHASE 1u                          // a chase ran longer than the number of points
#define TOPO_ERR_RETRY 2u                          // a union retried more often than there are points
#define TOPO_ERR_LABEL 4u                          // a chase met a label that is no ancestor (negative, or above its point)
#define TOPO_TAG_LAYERED 3ll                       // the tag's second word after a layer labelling (else: region + 1)

// the 32 region bits of points p .. p + 31, zeros before the first point and past the bit string
static __device__ __forceinline__ unsigned topo_bits_at(const unsigned* __restrict__ bits, long long words, long long p) {
    if (p >= 0) return mesh_bits_at(bits, words, p);
    if (p <= -32) return 0u;
    return bits[0] << (unsigned)(-p);
}

// the rows a word lies in: `in` its points in the grid, `start` / `end` the first / last point of a row, `jfirst` / `jlast`
// points of the first / last row of a layer (2-D: of the grid), `ifirst` points of the first layer (3-D) — the masks of
// mesh_valid, for predecessors instead of successors
struct TopoRows {
    unsigned in, start, end, jfirst, jlast, ifirst;
};
template <int D>
static __device__ __forceinline__ TopoRows topo_rows(const MeshGeom& g, long long p0) {
    TopoRows m = {0u, 0u, 0u, 0u, 0u, 0u};
    const long long end = p0 + 32 < g.n ? p0 + 32 : g.n;
    if (p0 >= end) return m;
    const long long nj = D == 3 ? g.d[1] : g.d[0];
    long long r = p0 / g.rowlen, rs = r * g.rowlen;
    long long j = D == 3 ? r % nj : r, i = D == 3 ? r / nj : 0;
    for (; rs < end; ++r, rs += g.rowlen) {
        const long long lo = rs > p0 ? rs - p0 : 0, hi = (rs + g.rowlen < end ? rs + g.rowlen : end) - p0;
        const unsigned seg = mesh_span(lo, hi);
        m.in |= seg;
        if (rs >= p0) m.start |= 1u << (rs - p0);
        const long long tail = rs + g.rowlen - 1 - p0;
        if (tail < 32) m.end |= 1u << tail;
        if (j == 0) m.jfirst |= seg;
        if (j == nj - 1) m.jlast |= seg;
        if (D == 3 && i == 0) m.ifirst |= seg;
        if (++j == nj) {
            j = 0;
            ++i;
        }
    }
    return m;
}

// the valid points of word w
static __device__ __forceinline__ unsigned topo_in(long long n, long long w) {
    const long long left = n - w * 32;
    return left >= 32 ? 0xffffffffu : left > 0 ? mesh_span(0, left) : 0u;
}

// the region's bit string: the inside bits, or (region = outside) their complement, under the valid-point mask — every
// later pass may rely on zeros past n
__global__ __launch_bounds__(SDFK_TOPO_THREADS) void sdfk_topo_region_kernel(const unsigned* __restrict__ bits, long long n, bool outside,
                                                                             unsigned* __restrict__ rb) {
    const long long w = (long long)sdfk_bx() * SDFK_TOPO_THREADS + sdfk_tx();
    rb[w] = (outside ? ~bits[w] : bits[w]) & topo_in(n, w);
}

// init: one word per thread finds its run starts, the wave writes its 2048 labels as 32 coalesced rows of 64
__global__ __launch_bounds__(SDFK_TOPO_THREADS) void sdfk_topo_init_kernel(const unsigned* __restrict__ rb, MeshGeom g,
                                                                           int* __restrict__ label) {
    const long long w = (long long)sdfk_bx() * SDFK_TOPO_THREADS + sdfk_tx();
    const long long p0 = w * 32;
    const unsigned x = rb[w];
    const long long rowbeg = p0 / g.rowlen * g.rowlen;         // the row of the word's first point
    unsigned start = 0u;
    for (long long rs = rowbeg; rs < p0 + 32; rs += g.rowlen)
        if (rs >= p0) start |= 1u << (rs - p0);
    // run starts: a set bit whose predecessor is clear or ends the row before (bit 0 counts as one here)
    const unsigned st = x & ~((x << 1) & ~start);
    long long carry = p0;                                       // where the run of bit 0 starts
    if ((x & 1u) && !(start & 1u)) {
        // the run enters from the word before: back over the previous words' bits to the last clear bit of this row
        carry = rowbeg;
        for (long long v = w - 1; v >= (rowbeg >> 5); --v) {
            const long long v0 = v * 32;
            unsigned z = ~rb[v];
            if (v0 < rowbeg) z &= ~((1u << (rowbeg - v0)) - 1u);
            if (z) {
                carry = v0 + 32 - __clz(z);
                break;
            }
        }
    }
    const int lane = sdfk_tx() & 63;
    const long long wb = w - lane;
    for (int j = 0; j < 32; ++j) {
        const int sl = 2 * j + (lane >> 5), bit = lane & 31;
        const unsigned xs = __shfl(x, sl, 64), sts = __shfl(st, sl, 64);
        const int cs = __shfl((int)carry, sl, 64);
        const long long q0 = (wb + sl) * 32, p = q0 + bit;
        int v = -1;
        if (xs >> bit & 1u) {
            const int hb = 31 - __clz(sts & (0xffffffffu >> (31 - bit)));      // the run start at or below the bit
            v = hb == 0 ? cs : (int)(q0 + hb);
        }
        if (p < g.n) label[p] = v;
    }
}

// Labels are read with relaxed agent-scope atomic loads: other workgroups, on other XCDs, lower them while this one
// chases. A stale, larger value is still a correct ancestor (a label is only ever lowered, to a point of the same set);
// whether a link is made is decided by the value atomicMin returns, never by a load.
static __device__ __forceinline__ int topo_load(const int* label, long long i) {
    return __hip_atomic_load(label + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root above a: labels strictly decrease along the chase, so it ends within n steps; -1 when the cap is hit
static __device__ __forceinline__ int topo_find(const int* label, int a, long long cap, unsigned* err) {
    for (long long it = 0; it <= cap; ++it) {
        const int l = topo_load(label, a);
        if (l == a) return a;
        if (l < 0 || l > a) {
            atomicOr(err, TOPO_ERR_LABEL);
            return -1;
        }
        a = l;
    }
    atomicOr(err, TOPO_ERR_CHASE);
    return -1;
}

// join the sets of a and b: atomicMin of the smaller root onto the larger. When the larger was no root any more (the
// returned value is below it), its set hangs under that value: go on from there. The larger of the two roots strictly
// decreases from try to try.
static __device__ __forceinline__ void topo_union(int* label, int a, int b, long long cap, unsigned* err) {
    for (long long it = 0; it <= cap; ++it) {
        a = topo_find(label, a, cap, err);
        b = topo_find(label, b, cap, err);
        if (a < 0 || b < 0 || a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(label + a, b);
        if (old == a) return;
        a = old;
    }
    atomicOr(err, TOPO_ERR_RETRY);
}

static __device__ __forceinline__ void topo_unions(int* label, unsigned first, long long p0, long long q0, long long cap,
                                                   unsigned* err) {
    while (first) {
        const int b = __builtin_ctz(first);
        first &= first - 1u;
        topo_union(label, (int)(p0 + b), (int)(q0 + b), cap, err);
    }
}

// merge: one word per thread; for every backward neighbour row (the same row at (dz, dy) before (0, 0)) the stretches
// where the two rows touch. A point and its left neighbour are one run already, and so are their partners in the other
// row: only the first bit of a stretch needs a union. Full connectivity adds the partners one column to the left and to
// the right, each a union of its own where the partner in the same column is missing (the three partners of a point may
// be two different runs).
template <int D, bool FULL>
__global__ __launch_bounds__(SDFK_TOPO_THREADS) void sdfk_topo_merge_kernel(const unsigned* __restrict__ rb, MeshGeom g, int* label,
                                                                            long long cap, unsigned* err) {
    const long long w = (long long)sdfk_bx() * SDFK_TOPO_THREADS + sdfk_tx();
    const long long p0 = w * 32;
    const unsigned x = rb[w];
    if (!x) return;
    const TopoRows m = topo_rows<D>(g, p0);
    constexpr int NR = D == 2 ? 1 : FULL ? 4 : 2;
    const long long sj = g.rowlen, si = D == 3 ? g.s[0] : 0;
    const long long off[4] = {sj, si, si + sj, si - sj};
    const unsigned has[4] = {~m.jfirst, ~m.ifirst, ~m.ifirst & ~m.jfirst, ~m.ifirst & ~m.jlast};
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const unsigned ok = x & m.in & has[r];
        if (!ok) continue;
        const long long q0 = p0 - off[r];
        const unsigned ov = ok & topo_bits_at(rb, g.words, q0);
        topo_unions(label, ov & ~((ov << 1) & ~m.start), p0, q0, cap, err);
        if (FULL) {
            const unsigned left = ok & topo_bits_at(rb, g.words, q0 - 1) & ~m.start & ~ov;
            const unsigned right = ok & topo_bits_at(rb, g.words, q0 + 1) & ~m.end & ~ov;
            topo_unions(label, left, p0, q0 - 1, cap, err);
            topo_unions(label, right, p0, q0 + 1, cap, err);
        }
    }
}

// compress: every point of the region reads its root. Other lanes store roots meanwhile; old or new, what a load sees
// is an ancestor.
__global__ __launch_bounds__(256) void sdfk_topo_compress_kernel(int* label, long long n, long long cap, unsigned* err) {
    const long long p = (long long)sdfk_bx() * 256 + sdfk_tx();
    if (p >= n) return;
    const int l = topo_load(label, p);
    if (l < 0) return;
    const int r = topo_find(label, l, cap, err);
    if (r >= 0 && r != l) label[p] = r;
}

// number: the root flags of the tile's words (a wave reads its 2048 labels as 32 coalesced rows of 64 and ballots),
// the roots per tile, the in-tile prefix per word
__global__ __launch_bounds__(SDFK_TOPO_THREADS) void sdfk_topo_number_kernel(const int* __restrict__ label, MeshGeom g,
                                                                             unsigned long long* __restrict__ blk,
                                                                             unsigned* __restrict__ rootbits,
                                                                             unsigned* __restrict__ rootpre) {
    __shared__ unsigned wsum[SDFK_TOPO_THREADS / 64];
    const long long w = (long long)sdfk_bx() * SDFK_TOPO_THREADS + sdfk_tx();
    const int lane = sdfk_tx() & 63;
    const long long wb = w - lane;
    unsigned mine = 0u;
    for (int j = 0; j < 32; ++j) {
        const long long p = wb * 32 + j * 64 + lane;
        const bool root = p < g.n && label[p] == (int)p;
        const unsigned long long all = __ballot(root);
        if (lane == 2 * j) mine = (unsigned)all;
        if (lane == 2 * j + 1) mine = (unsigned)(all >> 32);
    }
    unsigned total;
    const unsigned pre = mesh_block_exclusive(__popc(mine), &total, wsum);
    rootbits[w] = mine;
    rootpre[w] = pre;
    if (sdfk_tx() == 0) blk[sdfk_bx()] = total;
}

// the id of root r (after the scan of the tile counts)
static __device__ __forceinline__ long long topo_root_id(const unsigned long long* __restrict__ blk, const unsigned* __restrict__ rootbits,
                                                         const unsigned* __restrict__ rootpre, long long r) {
    const long long rw = r >> 5;
    return (long long)blk[r / SDFK_SEL_TILE] + rootpre[rw] + __popc(rootbits[rw] & ((1u << ((unsigned)r & 31u)) - 1u));
}

__global__ __launch_bounds__(256) void sdfk_topo_relabel_kernel(int* __restrict__ label, long long n,
                                                                const unsigned long long* __restrict__ blk,
                                                                const unsigned* __restrict__ rootbits,
                                                                const unsigned* __restrict__ rootpre) {
    const long long p = (long long)sdfk_bx() * 256 + sdfk_tx();
    if (p >= n) return;
    const int l = label[p];
    if (l >= 0) label[p] = (int)topo_root_id(blk, rootbits, rootpre, l);
}

// ---- records ---------------------------------------------------------------------------------------------------------
struct TopoRecords {
    long long* first;             // K
    unsigned long long* size;     // K
    int* lower;                   // K x D
    int* upper;                   // K x D
    unsigned* border;             // K
};
template <int D>
struct TopoAcc {
    int id, cnt, lo[D], hi[D];
    unsigned border;
};
template <int D>
static __device__ __forceinline__ void topo_flush(const TopoAcc<D>& a, const TopoRecords& rec, long long K) {
    if (a.id < 0 || a.id >= K) return;
    atomicAdd(rec.size + a.id, (unsigned long long)a.cnt);
    // box and border only move one way: an atomic that cannot change the word is left out. What the load sees may be
    // stale, that is further from the final value than the word is now — then the atomic is issued and decides.
#pragma unroll
    for (int o = 0; o < D; ++o) {
        int* lo = rec.lower + (long long)a.id * D + o;
        int* hi = rec.upper + (long long)a.id * D + o;
        if (a.lo[o] < __hip_atomic_load(lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(lo, a.lo[o]);
        if (a.hi[o] > __hip_atomic_load(hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(hi, a.hi[o]);
    }
    if (a.border && !__hip_atomic_load(rec.border + a.id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(rec.border + a.id, 1u);
}

// reduce: one word per thread, its row runs one after the other (labels are ids by now). `first` comes from the root
// flags with plain stores: every id has exactly one root. Runs of one component are added up in registers; when all the
// runs of a wave belong to one component the wave adds once. INPLANE (sdfk_layers.inc, D = 3): the border is the four
// in-plane edges of a layer alone — lying in the first or last layer does not count.
template <int D, bool INPLANE = false>
__global__ __launch_bounds__(SDFK_TOPO_THREADS) void sdfk_topo_reduce_kernel(const unsigned* __restrict__ rb, const int* __restrict__ label,
                                                                             MeshGeom g, const unsigned long long* __restrict__ blk,
                                                                             const unsigned* __restrict__ rootbits,
                                                                             const unsigned* __restrict__ rootpre, long long K,
                                                                             TopoRecords rec) {
    const long long w = (long long)sdfk_bx() * SDFK_TOPO_THREADS + sdfk_tx();
    const long long p0 = w * 32;
    unsigned roots = rootbits[w];
    long long rid = (long long)blk[sdfk_bx()] + rootpre[w];
    while (roots) {
        const int b = __builtin_ctz(roots);
        roots &= roots - 1u;
        if (rid < K) rec.first[rid] = p0 + b;
        ++rid;
    }
    TopoAcc<D> acc;
    acc.id = -1;
    acc.cnt = 0;
    acc.border = 0u;
#pragma unroll
    for (int o = 0; o < D; ++o) {
        acc.lo[o] = 0x7fffffff;
        acc.hi[o] = -1;
    }
    unsigned x = rb[w];
    if (x) {
        const TopoRows m = topo_rows<D>(g, p0);
        const long long nj = D == 3 ? g.d[1] : g.d[0];
        long long row = p0 / g.rowlen, col = p0 - row * g.rowlen;
        int at = 0;
        while (x) {
            const int b = __builtin_ctz(x);
            const unsigned y = x >> b, e = m.end >> b;
            int len = ~y ? __builtin_ctz(~y) : 32 - b;
            if (e && __builtin_ctz(e) + 1 < len) len = __builtin_ctz(e) + 1;
            x &= ~mesh_span(b, b + len);
            col += b - at;
            at = b;
            while (col >= g.rowlen) {
                col -= g.rowlen;
                ++row;
            }
            const int id = label[p0 + b];
            if (id != acc.id) {
                topo_flush<D>(acc, rec, K);
                acc.id = id;
                acc.cnt = 0;
                acc.border = 0u;
#pragma unroll
                for (int o = 0; o < D; ++o) {
                    acc.lo[o] = 0x7fffffff;
                    acc.hi[o] = -1;
                }
            }
            int c[3];
            if (D == 3) {
                c[0] = (int)(row / nj);
                c[1] = (int)(row - (long long)c[0] * nj);
            } else {
                c[0] = (int)row;
            }
            c[D - 1] = (int)col;
            const int c1 = (int)col + len - 1;
            acc.cnt += len;
#pragma unroll
            for (int o = 0; o < D - 1; ++o) {
                acc.lo[o] = min(acc.lo[o], c[o]);
                acc.hi[o] = max(acc.hi[o], c[o]);
                if ((!INPLANE || o > 0) && (c[o] == 0 || c[o] == g.d[o] - 1)) acc.border = 1u;
            }
            acc.lo[D - 1] = min(acc.lo[D - 1], c[D - 1]);
            acc.hi[D - 1] = max(acc.hi[D - 1], c1);
            if (col == 0 || c1 == g.rowlen - 1) acc.border = 1u;
        }
    }
    // what is left in the registers: one add per wave when every lane that has something has the same component
    const unsigned long long have = __ballot(acc.id >= 0);
    if (!have) return;
    const int ref = __shfl(acc.id, __builtin_ctzll(have), 64);
    if (__ballot(acc.id >= 0 && acc.id != ref)) {
        topo_flush<D>(acc, rec, K);
        return;
    }
    for (int d = 32; d > 0; d >>= 1) {
        acc.cnt += __shfl_xor(acc.cnt, d, 64);
        acc.border |= __shfl_xor(acc.border, d, 64);
#pragma unroll
        for (int o = 0; o < D; ++o) {
            acc.lo[o] = min(acc.lo[o], __shfl_xor(acc.lo[o], d, 64));
            acc.hi[o] = max(acc.hi[o], __shfl_xor(acc.hi[o], d, 64));
        }
    }
    acc.id = ref;
    if ((sdfk_tx() & 63) == 0) topo_flush<D>(acc, rec, K);
}

// ---- component moments: per id the sums of 1, i_a and i_a i_b over its points, from the label array alone ------------
// Definition: aegolius_amd/topology.py ("Component moments") and DESIGN §4.24. Row k of `sums` holds, in uint64,
//   3-D: N, I0, I1, I2, I00, I01, I02, I11, I12, I22        2-D: N, I0, I1, I00, I01, I11
// over the points with label k. Integer adds only: the rows do not depend on the order of the waves. The launcher refuses
// grids on which a sum could wrap (n (d_a - 1)(d_b - 1) >= 2^63), so no partial sum here can either.
// The labels are walked directly: the scratch of the labelling (the region's bits, the root flags) is gone when a caller
// holds labels only, and a bit string rebuilt from label >= 0 would cost a pass and n / 8 bytes to save nothing — the
// labels have to be read for the ids anyway, and runs found from the labels themselves are right for ANY label array,
// also one in which two neighbours of a row carry different ids. A wave takes a stretch of consecutive steps of 1024
// labels; in a step a lane owns 16 consecutive labels, four 16-byte loads that are all in flight together (the wave's 64
// lanes cover 4 KiB without a gap, every line is used whole). A quad whose four labels agree within one row is one run,
// any other quad is walked point by point. Runs enter in closed form (topo_run_sums); the runs of one grid row are kept as
// (sum 1, sum c, sum c^2) and multiplied by the leading indices when the row or the id changes. Accumulation, as in the
// reduce kernel but per step: consecutive runs of one component add up in the lane's registers and a lane that meets
// another id adds its sums to the row with 64-bit atomics; at the end of a step the lanes' sums are folded across the
// wave, once per component the lanes hold, into the wave's carry, which reaches memory when the wave moves on to another
// component or ends: a solid costs one set of adds per wave, not per lane or step. (Lanes that kept their sums from step
// to step, striding over the array, met another component at almost every step and flushed one by one: 92 ms on cfg 2
// at 513^3 against 3.6 ms for the reduce pass.)
#define SDFK_TOPO_MOM_THREADS 256
#define SDFK_TOPO_MOM_QUADS 4                      // 16-byte loads of a lane per step
#define SDFK_TOPO_MOM_BLOCKS 2048                  // at most: a wave takes consecutive steps
#define TOPO_ERR_ID 8u                             // a label that is neither -1 nor an id below K

struct TopoRun {
    unsigned long long s0, s1, s2;                 // sums of 1, c, c^2 over columns
};
// sum of m^2 for 0 <= m <= top: the numerator is below 1.5 n (d - 1)^2 < 2^64 on every grid the launcher lets through
// (top <= d - 1 and n >= 2 d)
static __device__ __forceinline__ unsigned long long topo_squares(unsigned long long top) {
    return top * (top + 1ull) * (2ull * top + 1ull) / 6ull;
}
// the columns c .. c + len - 1 (len >= 1), everything in 64 bits: c^2 passes 2^32 from 65,536 columns
static __device__ __forceinline__ void topo_run_sums(unsigned c, unsigned len, TopoRun& r) {
    const unsigned long long c64 = c, l64 = len;
    r.s0 += l64;
    r.s1 += l64 * (2ull * c64 + l64 - 1ull) / 2ull;
    r.s2 += topo_squares(c64 + l64 - 1ull) - (c ? topo_squares(c64 - 1ull) : 0ull);
}

template <int D>
struct TopoMomAcc {
    int id;                                        // -1: nothing yet
    unsigned a, b;                                 // the leading indices of the row `row` belongs to (2-D: a alone)
    TopoRun row;
    unsigned long long m[D == 3 ? 10 : 6];
};
template <int D>
static __device__ __forceinline__ void topo_mom_row(TopoMomAcc<D>& acc) {
    const unsigned long long a = acc.a, b = acc.b, s0 = acc.row.s0, s1 = acc.row.s1, s2 = acc.row.s2;
    if (D == 3) {
        acc.m[0] += s0;
        acc.m[1] += a * s0;
        acc.m[2] += b * s0;
        acc.m[3] += s1;
        acc.m[4] += a * a * s0;
        acc.m[5] += a * b * s0;
        acc.m[6] += a * s1;
        acc.m[7] += b * b * s0;
        acc.m[8] += b * s1;
        acc.m[9] += s2;
    } else {
        acc.m[0] += s0;
        acc.m[1] += a * s0;
        acc.m[2] += s1;
        acc.m[3] += a * a * s0;
        acc.m[4] += a * s1;
        acc.m[5] += s2;
    }
    acc.row.s0 = acc.row.s1 = acc.row.s2 = 0ull;
}
// m onto row `id` (an id below K, or -1: nothing); a sum that is zero — every sum of an index that is 0 — costs no atomic
template <int D>
static __device__ __forceinline__ void topo_mom_add(int id, const unsigned long long* m, unsigned long long* __restrict__ sums) {
    constexpr int NS = D == 3 ? 10 : 6;
    if (id < 0) return;
#pragma unroll
    for (int t = 0; t < NS; ++t)
        if (m[t]) atomicAdd(sums + (long long)id * NS + t, m[t]);
}
template <int D>
static __device__ __forceinline__ void topo_mom_flush(TopoMomAcc<D>& acc, long long K, unsigned long long* __restrict__ sums) {
    constexpr int NS = D == 3 ? 10 : 6;
    if (acc.id < K) topo_mom_add<D>(acc.id, acc.m, sums);
#pragma unroll
    for (int t = 0; t < NS; ++t) acc.m[t] = 0ull;
}
// one run of `len` points of `id` at columns c .. of the row (a, b). An id outside 0 .. K - 1 is never used as an index:
// it raises the error word and the run is left out.
template <int D>
static __device__ __forceinline__ void topo_mom_run(TopoMomAcc<D>& acc, int id, unsigned a, unsigned b, unsigned c, unsigned len,
                                                    long long K, unsigned long long* __restrict__ sums, unsigned* err) {
    if (id < 0 || id >= K) {
        atomicOr(err, TOPO_ERR_ID);
        return;
    }
    if (id != acc.id) {
        topo_mom_row<D>(acc);
        topo_mom_flush<D>(acc, K, sums);
        acc.id = id;
        acc.a = a;
        acc.b = b;
    } else if (a != acc.a || b != acc.b) {
        topo_mom_row<D>(acc);
        acc.a = a;
        acc.b = b;
    }
    topo_run_sums(c, len, acc.row);
}

static __device__ __forceinline__ unsigned long long topo_fold64(unsigned long long sum) {     // the wave's sum, in every lane
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned lo = (unsigned)sum, hi = (unsigned)(sum >> 32);
        sum += ((unsigned long long)__shfl_xor(hi, d, 64) << 32) | __shfl_xor(lo, d, 64);
    }
    return sum;
}

template <int D>
__global__ __launch_bounds__(SDFK_TOPO_MOM_THREADS) void sdfk_topo_moments_kernel(const int* __restrict__ label, MeshGeom g, long long K,
                                                                                  unsigned waves, unsigned long long* __restrict__ sums,
                                                                                  unsigned* err) {
    constexpr int NS = D == 3 ? 10 : 6, Q = SDFK_TOPO_MOM_QUADS;
    const unsigned n = (unsigned)g.n, rowlen = (unsigned)g.rowlen;           // (n <= 2^31 - 1)
    const unsigned nj = D == 3 ? (unsigned)g.d[1] : 1u;
    const unsigned lane = sdfk_tx() & 63u;
    const unsigned wave = sdfk_bx() * (SDFK_TOPO_MOM_THREADS / 64) + (sdfk_tx() >> 6);
    const unsigned steps = (n + 256u * Q - 1u) / (256u * Q);                  // 64 lanes x Q quads x 4 labels each
    const unsigned whole = n >> 2;                                           // whole quads: at least one (n >= 4)
    const int4* __restrict__ quad = reinterpret_cast<const int4*>(label);
    TopoMomAcc<D> acc;
    acc.id = -1;
    acc.a = acc.b = 0u;
    acc.row.s0 = acc.row.s1 = acc.row.s2 = 0ull;
#pragma unroll
    for (int t = 0; t < NS; ++t) acc.m[t] = 0ull;
    // the wave's carry: the folded sums of the component its last steps ended with (the same in every lane; lane 0 adds)
    int carry_id = -1;
    unsigned long long carry[NS];
#pragma unroll
    for (int t = 0; t < NS; ++t) carry[t] = 0ull;
    const unsigned share = (steps + waves - 1u) / waves;                     // consecutive steps per wave
    const unsigned first = min(wave * share, steps), last = min(first + share, steps);
    for (unsigned step = first; step < last; ++step) {                       // (wave-uniform trip count)
        // the loads first, without a branch between them (a quad past the last whole one reads that one again): all Q are
        // in flight before the first is looked at
        const unsigned q0 = (step * 64u + lane) * Q;
        int4 v[Q];
#pragma unroll
        for (int j = 0; j < Q; ++j) v[j] = quad[min(q0 + j, whole - 1u)];
#pragma unroll
        for (int j = 0; j < Q; ++j) {
            const unsigned p = (q0 + j) * 4u;                                // (below 2^31 + 1024)
            int l[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
            if (p + 4u > n) {                                                // the array's last, partial quad, and past it
                l[0] = p < n ? label[p] : -1;
                l[1] = p + 1u < n ? label[p + 1u] : -1;
                l[2] = p + 2u < n ? label[p + 2u] : -1;
                l[3] = -1;
            }
            if ((l[0] & l[1] & l[2] & l[3]) == -1) continue;                 // four times -1
            unsigned r = p / rowlen, col = p - r * rowlen, a, b = 0u;
            if (D == 3) {
                a = r / nj;
                b = r - a * nj;
            } else {
                a = r;
            }
            // the run (cur, row ra / rb, columns c0 .. c0 + len - 1) grows point by point and is handed on where the label
            // changes, a row starts or the quad ends (e == 4): one place, so that the unrolled loop over the quads stays
            // small. Four equal labels inside one row skip the walk.
            int cur = -1, e = 0;
            unsigned c0 = 0u, len = 0u, ra = a, rb = b;
            if (l[0] == l[1] && l[1] == l[2] && l[2] == l[3] && col + 3u < rowlen) {
                cur = l[0];
                c0 = col;
                len = 4u;
                e = 4;
            }
#pragma unroll 1
            for (; e <= 4; ++e) {
                const int le = e == 0 ? l[0] : e == 1 ? l[1] : e == 2 ? l[2] : e == 3 ? l[3] : -1;
                if (e == 4 || le != cur || col == 0u) {
                    if (len) topo_mom_run<D>(acc, cur, ra, rb, c0, len, K, sums, err);
                    cur = le;
                    c0 = col;
                    len = 0u;
                    ra = a;
                    rb = b;
                }
                if (cur != -1) ++len;
                if (++col == rowlen) {
                    col = 0u;
                    if (D == 3) {
                        if (++b == nj) {
                            b = 0u;
                            ++a;
                        }
                    } else {
                        ++a;
                    }
                }
            }
        }
        topo_mom_row<D>(acc);
        // the step's sums leave the lanes: one fold across the wave per component the lanes hold (one, where the 1024
        // labels lie in one component), into the carry; a carry of another component is added to its row first
        unsigned long long pending = __ballot(acc.id >= 0);
        while (pending) {                                                    // (wave-uniform)
            const int ref = __shfl(acc.id, __builtin_ctzll(pending), 64);
            const bool mine = acc.id == ref;
            if (ref != carry_id) {
                if (lane == 0u) topo_mom_add<D>(carry_id, carry, sums);
                carry_id = ref;
#pragma unroll
                for (int t = 0; t < NS; ++t) carry[t] = 0ull;
            }
#pragma unroll
            for (int t = 0; t < NS; ++t) carry[t] += topo_fold64(mine ? acc.m[t] : 0ull);
            pending &= ~__ballot(mine);
        }
        acc.id = -1;
#pragma unroll
        for (int t = 0; t < NS; ++t) acc.m[t] = 0ull;
    }
    if (lane == 0u) topo_mom_add<D>(carry_id, carry, sums);
}

// ---- cell counts: V, E, F, C of the cubical complex the inside points span -------------------------------------------
// A cell is in the complex iff all its corners are inside: per word the AND of the corner words (funnel shifts, as the
// mesh count pass) under the successor masks of mesh_valid; per workgroup one 64-bit add per counter.
template <int D>
__global__ __launch_bounds__(SDFK_TOPO_THREADS) void sdfk_topo_cells_kernel(const unsigned* __restrict__ bits, MeshGeom g,
                                                                            unsigned long long* __restrict__ out) {
    __shared__ unsigned red[4][SDFK_TOPO_THREADS / 64];
    const long long w = (long long)sdfk_bx() * SDFK_TOPO_THREADS + sdfk_tx();
    const long long p0 = w * 32;
    const unsigned b0 = bits[w] & topo_in(g.n, w);
    unsigned c[4] = {0u, 0u, 0u, 0u};
    if (b0) {
        unsigned valid[3], k[1 << D];
        mesh_valid<D>(g, p0, valid);
        mesh_corners<D>(bits, g, p0, b0, k);
        c[0] = __popc(b0);
#pragma unroll
        for (int a = 0; a < D; ++a) {
            const int ca = 1 << (D - 1 - a);
            c[1] += __popc(b0 & k[ca] & valid[a]);
#pragma unroll
            for (int b = a + 1; b < D; ++b) {
                const int cb = 1 << (D - 1 - b);
                c[2] += __popc(b0 & k[ca] & k[cb] & k[ca | cb] & valid[a] & valid[b]);
            }
        }
        if (D == 3) {
            unsigned all = b0 & valid[0] & valid[1] & valid[2];
#pragma unroll
            for (int q = 1; q < 8; ++q) all &= k[q];
            c[3] = __popc(all);
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        for (int d = 32; d > 0; d >>= 1) c[q] += __shfl_xor(c[q], d, 64);
    if ((sdfk_tx() & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) red[q][sdfk_tx() >> 6] = c[q];
    }
    __syncthreads();
    if (sdfk_tx() < 4) {
        unsigned long long t = 0;
        for (int v = 0; v < SDFK_TOPO_THREADS / 64; ++v) t += red[sdfk_tx()][v];
        if (t) atomicAdd(out + sdfk_tx(), t);
    }
}

// ---- label field: `inside` at the points of the kept ids, `outside` elsewhere ------------------------------------------
__global__ __launch_bounds__(256) void sdfk_topo_field_kernel(const int* __restrict__ label, long long n,
                                                              const unsigned char* __restrict__ keep, long long K, float inside,
                                                              float outside, float* __restrict__ out, long long step) {
    for (long long p = (long long)sdfk_bx() * 256 + sdfk_tx(); p < n; p += step) {
        const int l = label[p];
        out[p] = l >= 0 && l < K && keep[l] ? inside : outside;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// scratch: the mesh state of the geometry path (its record region holds the flag slots of the evaluation first, then the
// region's bit string | root flags | root prefixes, 12 of its 16 bytes per word) | control block: the error word, the
// four cell counters, and the tag {points, region of the last labelling + 1, its K} the later calls check.
// Per point: 1/8 B inside bits, 1/2 B record region (more where the flag slots need it: at most 1 B per point in all,
// as the mesh), 1/8 B unused prefixes; the labels (4 B per point) are the caller's.
struct TopoScratch {
    MeshScratch m;
    unsigned* rb;                 // the region's bits
    unsigned* rootbits;
    unsigned* rootpre;
    unsigned* err;
    unsigned long long* cells;    // 4
    long long* tag;               // 3
};
static size_t topo_layout(int D, const int64_t* dims, long long n, TopoScratch* sc, void* base) {
    size_t off = mesh_layout(n, mesh_naxis(D, dims, true), sc ? &sc->m : nullptr, base, mesh_flag_bytes(D, dims, n));
    const size_t o_c = off;
    off += 256;
    if (sc) {
        const long long words = sc->m.tiles * SDFK_TOPO_THREADS;
        sc->rb = reinterpret_cast<unsigned*>(sc->m.rec);
        sc->rootbits = sc->rb + words;
        sc->rootpre = sc->rb + 2 * words;
        char* c = static_cast<char*>(base) + o_c;
        sc->err = reinterpret_cast<unsigned*>(c);
        sc->cells = reinterpret_cast<unsigned long long*>(c + 64);
        sc->tag = reinterpret_cast<long long*>(c + 128);
    }
    return off;
}

struct TopoEvents {
    hipEvent_t e[SDFK_LABEL_PASSES + 1] = {};
    int n = 0;
    bool on = false;
    ~TopoEvents() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
    int start(float* pass_ms) {
        on = pass_ms != nullptr;
        if (!on) return 0;
        for (int k = 0; k < SDFK_LABEL_PASSES; ++k) pass_ms[k] = 0.0f;
        for (hipEvent_t& x : e) HIPCHK(hipEventCreate(&x));
        return 0;
    }
    int mark(hipStream_t stream) {
        if (on && n <= SDFK_LABEL_PASSES) HIPCHK(hipEventRecord(e[n++], stream));
        return 0;
    }
    int read(float* pass_ms) {                                   // (after the stream was waited for)
        if (on)
            for (int k = 0; k + 1 < n; ++k) HIPCHK(hipEventElapsedTime(&pass_ms[k], e[k], e[k + 1]));
        return 0;
    }
};

// the grid: 2 or 3 axes (n2 == 1: two), at most 2^31 - 1 points — labels are int32
static int topo_geom(int64_t n0, int64_t n1, int64_t n2, int* D, int64_t* dims, MeshGeom* g, const char* who) {
    if (n2 < 1) return fail(-1, std::string(who) + ": every axis needs 2 to 2^30 points (a 2-D grid has n2 = 1)");
    *D = n2 == 1 ? 2 : 3;
    dims[0] = n0;
    dims[1] = n1;
    dims[2] = n2;
    const int rc = mesh_geom(*D, dims, g, who);
    if (rc) return rc;
    if (g->n > 0x7fffffffll) return fail(-1, std::string(who) + ": more than 2^31 - 1 points (labels are 32-bit)");
    return 0;
}

// the inside bits of the source into the scratch: tables up, evaluation (or the selection's count kernel) to bits, the
// control block cleared and tagged
template <int D>
static int topo_bits(const MeshSrc& src, const float* const* ax, const int64_t* dims, const MeshGeom& g, float level,
                     const TopoScratch& sc, hipStream_t stream, const char* who) {
    long long at = 0;
    for (int a = 0; a < D; ++a) {
        HIPCHK(hipMemcpyAsync(sc.m.axes + at, ax[a], (size_t)dims[a] * sizeof(float), hipMemcpyHostToDevice, stream));
        at += dims[a];
    }
    if (src.prog) {
        if (D == 2) HIPCHK(hipMemsetAsync(sc.m.axes + at, 0, sizeof(float), stream));
        const int rc = mesh_eval_bits<D>(src, dims, g, sc.m, level, stream, who);
        if (rc) return rc;
    } else {
        hipLaunchKernelGGL(sdfk_select_count_kernel<true>, dim3((unsigned)((sc.m.tiles + SDFK_SEL_TPW - 1) / SDFK_SEL_TPW)),
                           dim3(SDFK_SEL_THREADS), 0, stream, src.field, g.n, sdfk_sel_key(level), sc.m.vblk, sc.m.bits);
    }
    HIPCHK(hipMemsetAsync(sc.err, 0, 256, stream));
    const long long tag[3] = {g.n, 0, 0};
    HIPCHK(hipMemcpyAsync(sc.tag, tag, sizeof(tag), hipMemcpyHostToDevice, stream));
    return 0;
}

static int topo_source(const MeshSrc& src, const float* ax0, int64_t n0, const float* ax1, int64_t n1, const float* ax2, int64_t n2,
                       float level, void* d_scratch, hipStream_t stream, const char* who, int* D, int64_t* dims, MeshGeom* g,
                       TopoScratch* sc) {
    if (!(src.field || src.prog) || !d_scratch) return fail(-1, std::string(who) + ": bad arguments");
    if ((uintptr_t)src.field & 15) return fail(-1, std::string(who) + ": the field must be 16-byte aligned");
    if ((uintptr_t)d_scratch & 255) return fail(-1, std::string(who) + ": the scratch must be 256-byte aligned");
    if (src.prog && src.prog->n_aux > 0)
        return fail(-1, std::string(who) + ": staged programs (auxiliary fields) are evaluated to a field first");
    if (!mesh_level_ok(level)) return fail(-1, std::string(who) + ": the level is NaN");
    int rc = topo_geom(n0, n1, n2, D, dims, g, who);
    if (rc) return rc;
    const float* ax[3] = {ax0, ax1, ax2};
    for (int a = 0; a < *D; ++a) {
        if (!ax[a]) return fail(-1, std::string(who) + ": axis table missing");
        for (long long i = 0; i + 1 < dims[a]; ++i)
            if (!(ax[a][i] < ax[a][i + 1])) return fail(-1, std::string(who) + ": axis tables must be strictly increasing");
    }
    topo_layout(*D, dims, g->n, sc, d_scratch);
    return *D == 3 ? topo_bits<3>(src, ax, dims, *g, level, *sc, stream, who) : topo_bits<2>(src, ax, dims, *g, level, *sc, stream, who);
}

template <int D>
static void topo_launch_merge(bool full, const unsigned* rb, const MeshGeom& g, int* label, unsigned* err, unsigned tiles,
                              hipStream_t stream) {
    const long long cap = g.n;
    if (full)
        hipLaunchKernelGGL((sdfk_topo_merge_kernel<D, true>), dim3(tiles), dim3(SDFK_TOPO_THREADS), 0, stream, rb, g, label, cap, err);
    else
        hipLaunchKernelGGL((sdfk_topo_merge_kernel<D, false>), dim3(tiles), dim3(SDFK_TOPO_THREADS), 0, stream, rb, g, label, cap, err);
}

typedef void (*TopoMerge)(bool full, const unsigned* rb, const MeshGeom& g, int* label, unsigned* err, unsigned tiles,
                          hipStream_t stream);

// the labelling of the bit string the scratch holds. ev: marked once already (before the bits); the marks made here end
// the passes bits (the region's bit string included), init, merge, compress, number. `merge`: another merge pass than the
// grid's own neighbourhood (sdfk_layers.inc: in-plane only); the tag then carries `kind` instead of region + 1.
static int topo_label(int D, const MeshGeom& g, const TopoScratch& sc, int connectivity, int region, int* d_labels, int64_t* count,
                      TopoEvents& ev, float* pass_ms, hipStream_t stream, const char* who, TopoMerge merge = nullptr,
                      long long kind = 0) {
    if (!d_labels || !count) return fail(-1, std::string(who) + ": bad arguments");
    if (connectivity != SDFK_CONNECT_FACES && connectivity != SDFK_CONNECT_FULL)
        return fail(-1, std::string(who) + ": connectivity is SDFK_CONNECT_FACES or SDFK_CONNECT_FULL");
    if (region != SDFK_REGION_INSIDE && region != SDFK_REGION_OUTSIDE)
        return fail(-1, std::string(who) + ": region is SDFK_REGION_INSIDE or SDFK_REGION_OUTSIDE");
    *count = 0;
    const unsigned tiles = (unsigned)sc.m.tiles, blocks = (unsigned)((g.n + 255) / 256);
    const bool full = connectivity == SDFK_CONNECT_FULL;
    const unsigned* rb = sc.rb;
    hipLaunchKernelGGL(sdfk_topo_region_kernel, dim3(tiles), dim3(SDFK_TOPO_THREADS), 0, stream, sc.m.bits, g.n,
                       region == SDFK_REGION_OUTSIDE, sc.rb);
    HIPCHK(hipMemsetAsync(sc.err, 0, sizeof(unsigned), stream));
    int rc = ev.mark(stream);
    if (rc) return rc;
    hipLaunchKernelGGL(sdfk_topo_init_kernel, dim3(tiles), dim3(SDFK_TOPO_THREADS), 0, stream, rb, g, d_labels);
    if ((rc = ev.mark(stream))) return rc;
    if (merge) merge(full, rb, g, d_labels, sc.err, tiles, stream);
    else if (D == 3) topo_launch_merge<3>(full, rb, g, d_labels, sc.err, tiles, stream);
    else topo_launch_merge<2>(full, rb, g, d_labels, sc.err, tiles, stream);
    if ((rc = ev.mark(stream))) return rc;
    hipLaunchKernelGGL(sdfk_topo_compress_kernel, dim3(blocks), dim3(256), 0, stream, d_labels, g.n, g.n, sc.err);
    if ((rc = ev.mark(stream))) return rc;
    hipLaunchKernelGGL(sdfk_topo_number_kernel, dim3(tiles), dim3(SDFK_TOPO_THREADS), 0, stream, d_labels, g, sc.m.vblk, sc.rootbits,
                       sc.rootpre);
    hipLaunchKernelGGL(sdfk_select_scan_kernel, dim3(1), dim3(1024), 0, stream, sc.m.vblk, (long long)tiles);
    hipLaunchKernelGGL(sdfk_topo_relabel_kernel, dim3(blocks), dim3(256), 0, stream, d_labels, g.n, sc.m.vblk, sc.rootbits, sc.rootpre);
    if ((rc = ev.mark(stream))) return rc;
    hipError_t e = hipGetLastError();
    unsigned long long K = 0;
    unsigned err = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&K, sc.m.vblk + tiles, 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&err, sc.err, sizeof(err), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(-6, std::string(who) + ": " + hipGetErrorString(e));
    if (err) return fail(-7, std::string(who) + ": an iteration cap was reached on the device (error word " + std::to_string(err) + ")");
    const long long tag[3] = {g.n, merge ? kind : region + 1, (long long)K};
    HIPCHK(hipMemcpy(sc.tag, tag, sizeof(tag), hipMemcpyHostToDevice));
    if ((rc = ev.read(pass_ms))) return rc;
    *count = (int64_t)K;
    return 0;
}

// the tag of the scratch against the grid: -> {points, region + 1, K}
static int topo_tag(const TopoScratch& sc, const MeshGeom& g, long long* tag, const char* who) {
    HIPCHK(hipMemcpy(tag, sc.tag, 3 * sizeof(long long), hipMemcpyDeviceToHost));
    if (tag[0] != g.n) return fail(-1, std::string(who) + ": the scratch does not hold the inside bits of that grid");
    return 0;
}

template <int D>
static void topo_launch_cells(const TopoScratch& sc, const MeshGeom& g, hipStream_t stream) {
    hipLaunchKernelGGL(sdfk_topo_cells_kernel<D>, dim3((unsigned)sc.m.tiles), dim3(SDFK_TOPO_THREADS), 0, stream, sc.m.bits, g, sc.cells);
}
static int topo_cells(int D, const MeshGeom& g, const TopoScratch& sc, int64_t* counts, hipStream_t stream, const char* who) {
    if (!counts) return fail(-1, std::string(who) + ": bad arguments");
    HIPCHK(hipMemsetAsync(sc.cells, 0, 4 * sizeof(unsigned long long), stream));
    if (D == 3) topo_launch_cells<3>(sc, g, stream);
    else topo_launch_cells<2>(sc, g, stream);
    hipError_t e = hipGetLastError();
    static_assert(sizeof(int64_t) == sizeof(unsigned long long), "counters are copied as they are");
    if (e == hipSuccess) e = hipMemcpyAsync(counts, sc.cells, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(-6, std::string(who) + ": " + hipGetErrorString(e));
    return 0;
}

extern "C" size_t sdfk_label_scratch(int64_t n0, int64_t n1, int64_t n2) {
    if (n0 < 1 || n1 < 1 || n2 < 1) return 512;
    const int64_t dims[3] = {n0, n1, n2};
    return topo_layout(n2 == 1 ? 2 : 3, dims, n0 * n1 * n2, nullptr, nullptr);
}

extern "C" int sdfk_field_label(const float* d_field, const float* ax0, int64_t n0, const float* ax1, int64_t n1, const float* ax2,
                                int64_t n2, float level, int connectivity, int region, int32_t* d_labels, int64_t* count,
                                void* d_scratch, float* pass_ms, void* stream_) {
    const char* who = "sdfk_field_label";
    hipStream_t stream = (hipStream_t)stream_;
    TopoEvents ev;
    int rc = ev.start(pass_ms);
    if (rc || (rc = ev.mark(stream))) return rc;
    int D;
    int64_t dims[3];
    MeshGeom g;
    TopoScratch sc;
    rc = topo_source(MeshSrc{d_field, nullptr, 0}, ax0, n0, ax1, n1, ax2, n2, level, d_scratch, stream, who, &D, dims, &g, &sc);
    if (rc) return rc;
    return topo_label(D, g, sc, connectivity, region, d_labels, count, ev, pass_ms, stream, who);
}

extern "C" int sdfk_eval_grid_label(sdfk_program* p, const float* ax0, int64_t n0, const float* ax1, int64_t n1, const float* ax2,
                                    int64_t n2, float level, int connectivity, int region, int32_t* d_labels, int64_t* count,
                                    void* d_scratch, float* pass_ms, void* stream_, int mode) {
    const char* who = "sdfk_eval_grid_label";
    if (!p) return fail(-1, std::string(who) + ": null program");
    hipStream_t stream = (hipStream_t)stream_;
    TopoEvents ev;
    int rc = ev.start(pass_ms);
    if (rc || (rc = ev.mark(stream))) return rc;
    int D;
    int64_t dims[3];
    MeshGeom g;
    TopoScratch sc;
    rc = topo_source(MeshSrc{nullptr, p, mode}, ax0, n0, ax1, n1, ax2, n2, level, d_scratch, stream, who, &D, dims, &g, &sc);
    if (rc) return rc;
    return topo_label(D, g, sc, connectivity, region, d_labels, count, ev, pass_ms, stream, who);
}

extern "C" int sdfk_label_bits(int64_t n0, int64_t n1, int64_t n2, int connectivity, int region, int32_t* d_labels, int64_t* count,
                               void* d_scratch, float* pass_ms, void* stream_) {
    const char* who = "sdfk_label_bits";
    if (!d_scratch || ((uintptr_t)d_scratch & 255)) return fail(-1, std::string(who) + ": the scratch must be 256-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    int D;
    int64_t dims[3];
    MeshGeom g;
    int rc = topo_geom(n0, n1, n2, &D, dims, &g, who);
    if (rc) return rc;
    TopoScratch sc;
    topo_layout(D, dims, g.n, &sc, d_scratch);
    long long tag[3];
    if ((rc = topo_tag(sc, g, tag, who))) return rc;
    TopoEvents ev;
    rc = ev.start(pass_ms);
    if (rc || (rc = ev.mark(stream))) return rc;
    return topo_label(D, g, sc, connectivity, region, d_labels, count, ev, pass_ms, stream, who);
}

template <int D, bool INPLANE = false>
static void topo_launch_reduce(const unsigned* rb, const int* label, const MeshGeom& g, const TopoScratch& sc, long long K,
                               const TopoRecords& rec, hipStream_t stream) {
    hipLaunchKernelGGL((sdfk_topo_reduce_kernel<D, INPLANE>), dim3((unsigned)sc.m.tiles), dim3(SDFK_TOPO_THREADS), 0, stream, rb, label, g,
                       sc.m.vblk, sc.rootbits, sc.rootpre, K, rec);
}

// the records of the labelling the scratch holds; layered: a layer labelling (sdfk_layers.inc), with the in-plane border
static int topo_finish(int64_t n0, int64_t n1, int64_t n2, int64_t count, const int32_t* d_labels, int64_t* first, int64_t* sizes,
                       int32_t* lower, int32_t* upper, int32_t* border, void* d_scratch, void* stream_, bool layered, const char* who) {
    if (!d_scratch || ((uintptr_t)d_scratch & 255)) return fail(-1, std::string(who) + ": the scratch must be 256-byte aligned");
    if (!d_labels || count < 0 || (count && (!first || !sizes || !lower || !upper || !border)))
        return fail(-1, std::string(who) + ": bad arguments");
    hipStream_t stream = (hipStream_t)stream_;
    int D;
    int64_t dims[3];
    MeshGeom g;
    int rc = topo_geom(n0, n1, n2, &D, dims, &g, who);
    if (rc) return rc;
    TopoScratch sc;
    topo_layout(D, dims, g.n, &sc, d_scratch);
    long long tag[3];
    if ((rc = topo_tag(sc, g, tag, who))) return rc;
    if (tag[1] < 1 || tag[2] != count) return fail(-1, std::string(who) + ": the scratch does not hold a labelling of that size");
    if (layered != (tag[1] == TOPO_TAG_LAYERED))
        return fail(-1, std::string(who) + (layered ? ": the scratch does not hold a layer labelling" : ": the scratch holds a layer labelling"));
    if (count == 0) return 0;
    const long long K = count;
    const size_t b8 = mesh_align((size_t)K * 8), bD = mesh_align((size_t)K * D * 4), b4 = mesh_align((size_t)K * 4);
    Scratch own;
    if (own.get(nullptr, 2 * b8 + 2 * bD + b4)) return fail(-5, std::string(who) + ": out of device memory (the records)");
    char* base = static_cast<char*>(own.p);
    TopoRecords rec;
    rec.first = reinterpret_cast<long long*>(base);
    rec.size = reinterpret_cast<unsigned long long*>(base + b8);
    rec.lower = reinterpret_cast<int*>(base + 2 * b8);
    rec.upper = reinterpret_cast<int*>(base + 2 * b8 + bD);
    rec.border = reinterpret_cast<unsigned*>(base + 2 * b8 + 2 * bD);
    HIPCHK(hipMemsetAsync(rec.first, 0, 2 * b8, stream));
    HIPCHK(hipMemsetAsync(rec.lower, 0x7f, bD, stream));          // above every index: an axis has at most 2^30 points
    HIPCHK(hipMemsetAsync(rec.upper, 0xff, bD, stream));          // -1
    HIPCHK(hipMemsetAsync(rec.border, 0, b4, stream));
    if (layered) topo_launch_reduce<3, true>(sc.rb, d_labels, g, sc, K, rec, stream);
    else if (D == 3) topo_launch_reduce<3>(sc.rb, d_labels, g, sc, K, rec, stream);
    else topo_launch_reduce<2>(sc.rb, d_labels, g, sc, K, rec, stream);
    hipError_t e = hipGetLastError();
    static_assert(sizeof(int64_t) == sizeof(long long), "records are copied as they are");
    if (e == hipSuccess) e = hipMemcpyAsync(first, rec.first, (size_t)K * 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(sizes, rec.size, (size_t)K * 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(lower, rec.lower, (size_t)K * D * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(upper, rec.upper, (size_t)K * D * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(border, rec.border, (size_t)K * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(-6, std::string(who) + ": " + hipGetErrorString(e));
    return 0;
}

extern "C" int sdfk_label_finish(int64_t n0, int64_t n1, int64_t n2, int64_t count, const int32_t* d_labels, int64_t* first,
                                 int64_t* sizes, int32_t* lower, int32_t* upper, int32_t* border, void* d_scratch, void* stream_) {
    return topo_finish(n0, n1, n2, count, d_labels, first, sizes, lower, upper, border, d_scratch, stream_, false, "sdfk_label_finish");
}

template <int D>
static void topo_launch_moments(const int* label, const MeshGeom& g, long long K, unsigned long long* sums, unsigned* err,
                                hipStream_t stream) {
    const long long steps = (g.n + 256 * SDFK_TOPO_MOM_QUADS - 1) / (256 * SDFK_TOPO_MOM_QUADS);
    const int per = SDFK_TOPO_MOM_THREADS / 64;
    const unsigned blocks = (unsigned)std::min<long long>((steps + per - 1) / per, SDFK_TOPO_MOM_BLOCKS);
    hipLaunchKernelGGL(sdfk_topo_moments_kernel<D>, dim3(blocks), dim3(SDFK_TOPO_MOM_THREADS), 0, stream, label, g, K, blocks * per, sums,
                       err);
}

// the moment rows of a label array: nothing but the labels is needed, so any labelling a caller still holds will do
extern "C" int sdfk_label_moments(int64_t n0, int64_t n1, int64_t n2, const int32_t* d_labels, int64_t count, uint64_t* sums,
                                  void* d_scratch, void* stream_) {
    const char* who = "sdfk_label_moments";
    (void)d_scratch;                                            // (the labels are walked directly: no scratch is needed)
    if (!d_labels || count < 0 || (count && !sums)) return fail(-1, std::string(who) + ": bad arguments");
    if ((uintptr_t)d_labels & 15) return fail(-1, std::string(who) + ": the labels must be 16-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    int D;
    int64_t dims[3];
    MeshGeom g;
    const int rc = topo_geom(n0, n1, n2, &D, dims, &g, who);
    if (rc) return rc;
    if (count > g.n) return fail(-1, std::string(who) + ": more components than points");
    // no wrap: every sum is at most n (d_a - 1)(d_b - 1), the largest of which is n (d_max - 1)^2
    const int64_t dmax = std::max(dims[0], std::max(dims[1], D == 3 ? dims[2] : (int64_t)1));
    if ((unsigned __int128)g.n * (unsigned __int128)(dmax - 1) * (unsigned __int128)(dmax - 1) >= ((unsigned __int128)1 << 63)) {
        std::string grid = std::to_string(n0) + "x" + std::to_string(n1) + (D == 3 ? "x" + std::to_string(n2) : std::string());
        return fail(-2, std::string(who) + ": a 64-bit sum could wrap on the grid " + grid + " (points x (longest axis - 1)^2 >= 2^63)");
    }
    if (count == 0) return 0;
    const long long K = count;
    const int NS = D == 3 ? 10 : 6;
    const size_t rows = mesh_align((size_t)K * NS * 8);
    Scratch own;
    if (own.get(nullptr, rows + 256)) return fail(-5, std::string(who) + ": out of device memory (the moment rows)");
    unsigned long long* d_sums = static_cast<unsigned long long*>(own.p);
    unsigned* d_err = reinterpret_cast<unsigned*>(static_cast<char*>(own.p) + rows);
    HIPCHK(hipMemsetAsync(own.p, 0, rows + 256, stream));
    if (D == 3) topo_launch_moments<3>(d_labels, g, K, d_sums, d_err, stream);
    else topo_launch_moments<2>(d_labels, g, K, d_sums, d_err, stream);
    hipError_t e = hipGetLastError();
    unsigned err = 0;
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "rows are copied as they are");
    if (e == hipSuccess) e = hipMemcpyAsync(sums, d_sums, (size_t)K * NS * 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&err, d_err, sizeof(err), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(-6, std::string(who) + ": " + hipGetErrorString(e));
    if (err) return fail(-7, std::string(who) + ": the array holds labels that are neither -1 nor an id below " + std::to_string(K));
    return 0;
}

extern "C" int sdfk_field_cell_counts(const float* d_field, const float* ax0, int64_t n0, const float* ax1, int64_t n1,
                                      const float* ax2, int64_t n2, float level, int64_t* counts, void* d_scratch, void* stream_) {
    const char* who = "sdfk_field_cell_counts";
    hipStream_t stream = (hipStream_t)stream_;
    int D;
    int64_t dims[3];
    MeshGeom g;
    TopoScratch sc;
    const int rc = topo_source(MeshSrc{d_field, nullptr, 0}, ax0, n0, ax1, n1, ax2, n2, level, d_scratch, stream, who, &D, dims, &g, &sc);
    if (rc) return rc;
    return topo_cells(D, g, sc, counts, stream, who);
}

extern "C" int sdfk_eval_grid_cell_counts(sdfk_program* p, const float* ax0, int64_t n0, const float* ax1, int64_t n1,
                                          const float* ax2, int64_t n2, float level, int64_t* counts, void* d_scratch,
                                          void* stream_, int mode) {
    const char* who = "sdfk_eval_grid_cell_counts";
    if (!p) return fail(-1, std::string(who) + ": null program");
    hipStream_t stream = (hipStream_t)stream_;
    int D;
    int64_t dims[3];
    MeshGeom g;
    TopoScratch sc;
    const int rc = topo_source(MeshSrc{nullptr, p, mode}, ax0, n0, ax1, n1, ax2, n2, level, d_scratch, stream, who, &D, dims, &g, &sc);
    if (rc) return rc;
    return topo_cells(D, g, sc, counts, stream, who);
}

extern "C" int sdfk_label_field(const int32_t* d_labels, int64_t n, const unsigned char* keep, int64_t count, float inside,
                                float outside, float* d_out, void* stream_) {
    const char* who = "sdfk_label_field";
    if (!d_labels || !d_out || n < 1 || n > 0x7fffffffll || count < 0 || (count && !keep))
        return fail(-1, std::string(who) + ": bad arguments");
    hipStream_t stream = (hipStream_t)stream_;
    Scratch table;
    if (table.get(nullptr, (size_t)std::max<int64_t>(count, 1))) return fail(-5, std::string(who) + ": out of device memory (keep table)");
    if (count) HIPCHK(hipMemcpyAsync(table.p, keep, (size_t)count, hipMemcpyHostToDevice, stream));
    const long long blocks = std::min<long long>((n + 255) / 256, 1ll << 20);
    hipLaunchKernelGGL(sdfk_topo_field_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_labels, (long long)n,
                       static_cast<const unsigned char*>(table.p), (long long)count, inside, outside, d_out, blocks * 256);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(-6, std::string(who) + ": " + hipGetErrorString(e));
    return 0;
}
