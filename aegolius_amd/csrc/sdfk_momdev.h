// sdfk_momdev.h — mass properties of one program: the sample pass that adds up, over the sub-sample points of its entries
// that lie in the solid (f <= level), the ten integer moments
//     M = (N, U0, U1, U2, U00, U01, U02, U11, U12, U22),   terms 1, u_a, u_a u_b,   u_a = 2 (i_a k_a + j_a) + 1
// (the odd lattice coordinate of sub-sample j_a of grid point i_a; the definition: aegolius_amd/moments.py). Shared, like
// sdfk_occdev.h, by the interpreter kernel (sdfk_moments.inc) and, as embedded text, by the hiprtc-specialised one
// (SDFK_FL_MOMENTS), around the same plain field objects: both give the same integers. Comes after sdfk_occdev.h, whose
// grid description (sdfk_occgrid), entry sources (SdfkOccList, SdfkOccAll) and lane mapping it uses unchanged:
//     K >= 64: one entry (cell) per group of K / 64 rounds, lane l of round r evaluates sub-index s = 64 r + l;
//     K <  64: 64 / K consecutive entries per group in one round, lane l -> entry l / K, sub-index l % K;
//     s = (j0 k1 + j1) k2 + j2. Lanes past the last entry evaluate entry 0 and add nothing: control flow is wave-uniform.
//
// A wave owns the groups wave, wave + waves, ... Every lane keeps the ten sums of ITS sub-samples in registers (64-bit;
// u_a fits 32 bits and u_a = 0 stands for "outside", so a sample costs three selects, six v_mad_u64_u32 and four 64-bit
// adds on the lane's own SIMD); after the last group the wave folds the lanes by halves, once, and lane 0 stores the
// wave's partial — ten uint64, plain vector stores, no atomics, no LDS. The host adds the partials as exact integers, so
// the result does not depend on the order. The launcher makes sure that no partial can wrap:
//     groups of a wave * max(K, 64) * (2 n k)^2 < 2^63,   n k the longest axis in sub-samples (sdfk_moments.inc).
// (The other form — one ballot per round, the local sums of j_a and j_a j_b as popcounts of the ballot under constant lane
// masks — needs 46 64-bit popcounts per round for k = 8 on three axes, on the one scalar unit the four SIMDs of a CU share,
// or on the vector unit wherever the entry's lane segment differs per lane (K < 64))
#ifndef SDFK_MOMDEV_H
#define SDFK_MOMDEV_H

#define SDFK_MOM_SUMS 10

// the sum over the wave's lanes, valid in lane 0
static __device__ __forceinline__ unsigned long long sdfk_mom_fold(unsigned long long sum) {
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned lo = (unsigned)sum, hi = (unsigned)(sum >> 32);
        sum += ((unsigned long long)__shfl_down(hi, off) << 32) | __shfl_down(lo, off);
    }
    return sum;
}

// FIELD: float operator()(V3) const — the program at one point (SdfkInterpField, or SdfkSpecField around sdfk_point<float>)
// waves: the waves of the launch (4 per block); partial: SDFK_MOM_SUMS uint64 per wave, every one of them is written
template <typename SRC, typename FIELD>
static __device__ __forceinline__ void sdfk_mom_sample(const SRC& src, const FIELD& field, const sdfk_occgrid G, unsigned waves,
                                                       unsigned long long* __restrict__ partial) {
    const unsigned lane = sdfk_tx() & 63u;
    const unsigned long long wave = (unsigned long long)sdfk_bx() * (SDFK_OCC_BLOCK / 64) + (sdfk_tx() >> 6);
    const bool wide = G.K >= 64u;                               // wave-uniform (a kernel argument)
    const unsigned seg = wide ? 0u : lane >> G.lK;              // this lane's entry within the group
    const unsigned rounds = wide ? G.K >> 6 : 1u;
    const unsigned long long groups = wide ? src.n : (src.n + (64u >> G.lK) - 1ull) >> (6u - G.lK);
    unsigned long long m[SDFK_MOM_SUMS];
#pragma unroll
    for (int t = 0; t < SDFK_MOM_SUMS; ++t) m[t] = 0ull;
    for (unsigned long long group = wave; group < groups; group += waves) {   // (wave-uniform trip count)
        const unsigned long long entry = wide ? group : (group << (6u - G.lK)) + seg;
        const bool live = entry < src.n;
        const unsigned cell = sdfk_occ_cell(src, live ? entry : 0ull);
        unsigned long long i0;
        unsigned i1, i2;
        if (G.small) {                                          // (wave-uniform: a kernel argument)
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
        // u of sub-sample 0 of the cell, per axis (2 n k < 2^32: the launcher's check)
        const unsigned e0 = 2u * ((unsigned)i0 * G.k0) + 1u, e1 = 2u * (i1 * G.k1) + 1u, e2 = 2u * (i2 * G.k2) + 1u;
        for (unsigned r = 0; r < rounds; ++r) {                 // (wave-uniform trip count)
            const unsigned s = wide ? (r << 6) + lane : lane & (G.K - 1u);
            const unsigned j2 = s & (G.k2 - 1u), j1 = (s >> G.l2) & (G.k1 - 1u), j0 = s >> (G.l2 + G.l1);
            const float f = field(V3{p0[j0], p1[j1], p2[j2]});
            const bool in = live && sdfk_sel_key(f) <= G.level_key;
            const unsigned u0 = in ? e0 + 2u * j0 : 0u, u1 = in ? e1 + 2u * j1 : 0u, u2 = in ? e2 + 2u * j2 : 0u;
            m[0] += in ? 1ull : 0ull;
            m[1] += u0;
            m[2] += u1;
            m[3] += u2;
            m[4] += (unsigned long long)u0 * u0;
            m[5] += (unsigned long long)u0 * u1;
            m[6] += (unsigned long long)u0 * u2;
            m[7] += (unsigned long long)u1 * u1;
            m[8] += (unsigned long long)u1 * u2;
            m[9] += (unsigned long long)u2 * u2;
        }
    }
#pragma unroll
    for (int t = 0; t < SDFK_MOM_SUMS; ++t) {
        const unsigned long long total = sdfk_mom_fold(m[t]);
        if (lane == 0u) partial[wave * SDFK_MOM_SUMS + t] = total;
    }
}

#endif  // SDFK_MOMDEV_H
