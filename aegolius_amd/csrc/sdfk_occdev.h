// sdfk_occdev.h — sub-voxel occupancy of one program: the sample pass that counts, per grid cell, how many of its K = k^d
// sub-sample points lie in the solid (f <= level). Shared (like sdfk_raydev.h) by the interpreter sample kernel
// (sdfk_occupancy.inc) and, as embedded text, by the hiprtc-specialised one (SDFK_FL_OCCUPANCY): the lane mapping and the
// count are ONE piece of text, and the field objects are the ray flavour's plain ones, so both kernels give the same bits.
//
// The cell of grid point (i0, i1, i2) — flat index (i0 n1 + i1) n2 + i2, z fastest — has the sub-samples
//     (T0[i0 k0 + j0], T1[i1 k1 + j1], T2[i2 k2 + j2]),   sub-index s = (j0 k1 + j1) k2 + j2   (z fastest),
// T* the host's sub-sample tables (aegolius_amd.occupancy.sample_tables states the formula); an axis of one point has
// k = 1 and the single sample 0.0 (2-D grids). k is 1, 2, 4 or 8 on every other axis, so K divides 64 or is a multiple.
//
// One sub-sample per lane:
//     K >= 64: a wave owns one entry (cell) for K / 64 rounds, lane l of round r evaluates s = 64 r + l;
//     K <  64: a wave owns 64 / K consecutive entries in one round, lane l -> entry l / K, sample l % K.
// Entries are the cells of a list (SdfkOccList: the near cells the classify pass appended, in any order) or all cells of
// the slab (SdfkOccAll). The cell index -> (i0, i1, i2) is computed once per entry, in 64 bits unless the grid has fewer than 2^32 cells. Lanes past the last entry
// evaluate entry 0 (a valid point) and are masked out of the ballot, so control flow is wave-uniform and the interpreter's
// code words stay scalar loads. count = popcount of the ballot masked to the entry's lane segment, summed over the rounds;
// one lane per entry stores count / K (exact: K is a power of two <= 512) with a plain vector store. No LDS and no atomics:
// one add per wave to a 64-bit total was measured to BE the pass (every wave of the device on one address: 11 ns per wave,
// 8.6 ms for the 782 k near cells of cfg 2 at 513^3, 23 times the evaluations themselves), so the total is summed from the
// stored fractions afterwards (sdfk_occupancy.inc).
//
// "inside" is decided on the selection key (sdfk_access.h): f <= level as the host compares them, a NaN value outside.
#ifndef SDFK_OCCDEV_H
#define SDFK_OCCDEV_H

#define SDFK_OCC_BLOCK 256

struct sdfk_occgrid {
    const float* __restrict__ t0;      // sub-sample tables: n_a k_a entries
    const float* __restrict__ t1;
    const float* __restrict__ t2;
    unsigned n1, n2;                   // cells along axes 1 and 2
    unsigned k1, k2;                   // sub-samples along axes 0, 1, 2: k0 = K / (k1 k2)
    unsigned k0;
    unsigned l1, l2;                   // log2 of k1, k2
    unsigned K, lK;                    // k0 k1 k2 and its log2
    float inv_K;                       // 1 / K (a power of two: count * inv_K is exact)
    unsigned level_key;                // sdfk_sel_key(level)
    unsigned small;                    // the grid has fewer than 2^32 cells: 32-bit index arithmetic
    long long first;                   // flat index of the slab's cell 0
};

struct SdfkOccList {                   // entry e = cell list[e] of the slab
    const unsigned* __restrict__ list;
    unsigned long long n;
};
struct SdfkOccAll {                    // entry e = cell e of the slab
    unsigned long long n;
};
static __device__ __forceinline__ unsigned sdfk_occ_cell(const SdfkOccList& s, unsigned long long e) { return s.list[e]; }
static __device__ __forceinline__ unsigned sdfk_occ_cell(const SdfkOccAll&, unsigned long long e) { return (unsigned)e; }

// FIELD: float operator()(V3) const — the program at one point (SdfkInterpField, or SdfkSpecField around sdfk_point<float>)
// out: the slab's fractions (cell c of the slab at out[c])
template <typename SRC, typename FIELD>
static __device__ __forceinline__ void sdfk_occ_sample(const SRC& src, const FIELD& field, const sdfk_occgrid G,
                                                       float* __restrict__ out) {
    const unsigned lane = sdfk_tx() & 63u;
    const unsigned long long wave = (unsigned long long)sdfk_bx() * (SDFK_OCC_BLOCK / 64) + (sdfk_tx() >> 6);
    const bool wide = G.K >= 64u;                               // wave-uniform (a kernel argument)
    const unsigned seg = wide ? 0u : lane >> G.lK;              // this lane's entry within the wave
    const unsigned long long entry = wide ? wave : (wave << (6u - G.lK)) + seg;
    const bool live = entry < src.n;
    const unsigned cell = sdfk_occ_cell(src, live ? entry : 0ull);
    unsigned long long i0;
    unsigned i1, i2;
    if (G.small) {                                              // (wave-uniform: a kernel argument)
        const unsigned flat = (unsigned)G.first + cell, row = flat / G.n2, q = row / G.n1;
        i2 = flat - row * G.n2;
        i1 = row - q * G.n1;
        i0 = q;
    } else {
        const unsigned long long flat = (unsigned long long)G.first + cell, row = flat / G.n2;
        i2 = (unsigned)(flat - row * G.n2);
        i0 = row / G.n1;
        i1 = (unsigned)(row - i0 * G.n1);
    }
    const float* __restrict__ p0 = G.t0 + i0 * G.k0;
    const float* __restrict__ p1 = G.t1 + (unsigned long long)i1 * G.k1;
    const float* __restrict__ p2 = G.t2 + (unsigned long long)i2 * G.k2;
    const unsigned long long mine = wide ? ~0ull : ((1ull << G.K) - 1ull) << (seg << G.lK);
    const unsigned rounds = wide ? G.K >> 6 : 1u;
    unsigned count = 0u;
    for (unsigned r = 0; r < rounds; ++r) {                     // (wave-uniform trip count)
        const unsigned s = wide ? (r << 6) + lane : lane & (G.K - 1u);
        const unsigned j2 = s & (G.k2 - 1u), j1 = (s >> G.l2) & (G.k1 - 1u), j0 = s >> (G.l2 + G.l1);
        const float f = field(V3{p0[j0], p1[j1], p2[j2]});
        const unsigned long long in = __ballot(live && sdfk_sel_key(f) <= G.level_key);
        count += (unsigned)__popcll(in & mine);
    }
    if (live && (wide ? lane == 0u : (lane & (G.K - 1u)) == 0u)) out[cell] = (float)count * G.inv_K;
}

#endif  // SDFK_OCCDEV_H
